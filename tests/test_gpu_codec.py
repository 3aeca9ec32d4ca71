"""GPU parity (-m gpu) of the RLE codec on tables (csrc/codec.hip): rle_from_string, rle_area_bbox, rle_to_string, rle_decode and
the cocoeval route through them. Every comparison is exact (integer / byte work). References: tests/golden/codec.npz and rle.npz
(the reference's own codec) and the numpy readers image.rle_counts / image.rle_decode / cocoeval._rle_area_bbox, which
tests/test_codec_host.py pins to the same fixture. Outputs are pre-filled with a poison value where the test owns the buffers
(the entry points are then called through the ctypes binding, as ops_coco.py calls them)."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_codec_host import codec_cases
from test_cocoeval_host import golden_inputs, same_eval_img
from test_gpu_rle import np_string
from test_rle_host import golden_cases as rle_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISON = 0x5A5A5A5A
BAD_BYTE, LONG_TOKEN, OPEN_TOKEN, BAD_SIZE, EMPTY_RUN, PIXEL_SUM = 1, 2, 4, 8, 16, 32


@pytest.fixture(scope="module")
def ops():
    from maskrcnn_amd import ops as o
    return o


@pytest.fixture(scope="module")
def cases():
    return codec_cases()


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def from_strings(strs, hs, ws, capacity, prefix=b""):
    """mrcnn_rle_from_string on poison-filled outputs → numpy (num_runs, counts uint32 [n,capacity], status). prefix: bytes in
    front of the first string (str_off[0] = len(prefix))."""
    from maskrcnn_amd import _lib
    n = len(strs)
    data = dev(np.frombuffer(prefix + b"".join(strs), np.uint8).copy())
    off = dev(len(prefix) + np.concatenate([[0], np.cumsum([len(s) for s in strs])]), np.int64)
    h, w = dev(hs, np.int32), dev(ws, np.int32)
    num_runs = torch.full((n,), POISON, dtype=torch.int32, device=DEV)
    status = torch.full((n,), POISON, dtype=torch.int32, device=DEV)
    counts = torch.full((n, capacity), POISON, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib.mrcnn_rle_from_string(data.data_ptr() if data.numel() else None, data.numel(), off.data_ptr(), h.data_ptr(),
                                              w.data_ptr(), n, capacity, num_runs.data_ptr(), counts.data_ptr(), status.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
    return num_runs.cpu().numpy(), counts.cpu().numpy().view(np.uint32), status.cpu().numpy()


def expected_status(cnts, h, w):
    st = 0
    if cnts.size > 1 and not cnts[1:].all():
        st |= EMPTY_RUN
    if int(cnts.astype(np.int64).sum()) != h * w:
        st |= PIXEL_SUM
    return st


def check_rows(got, strs, hs, ws, capacity, label=""):
    """Every row against image.rle_counts: num_runs, the counts, the status bits, and poison past num_runs."""
    from maskrcnn_amd import image
    num_runs, counts, status = got
    for i, s in enumerate(strs):
        want = image.rle_counts(s)
        assert num_runs[i] == want.size, (label, i)
        if want.size > capacity:
            assert status[i] == 0 and (counts[i] == POISON).all(), (label, i)
            continue
        assert np.array_equal(counts[i, :want.size], want), (label, i)
        assert (counts[i, want.size:] == POISON).all(), (label, i)
        assert status[i] == expected_status(want, hs[i], ws[i]), (label, i, status[i])


def table(rows, capacity=None, fill=0):
    """uint32 run lists → (num_runs, counts) device tensors, rows padded with `fill`."""
    capacity = capacity or max(1, max(len(r) for r in rows))
    t = np.full((len(rows), capacity), fill, dtype=np.uint32)
    for i, r in enumerate(rows):
        t[i, :len(r)] = r
    return dev([len(r) for r in rows], np.int32), dev(t.view(np.int32))


def seeded_counts(rng, runs):
    """A run list with differences of mixed sizes (1 to 4 characters each), every run in [1, 2^27)."""
    c = []
    for m in range(runs):
        prev = c[m - 2] if m > 2 else 0
        mag = int(rng.integers(0, 1 << int(rng.choice([4, 9, 14, 19]))))
        x = -mag if prev - mag >= 1 and (rng.random() < .5 or prev + mag >= 1 << 27) else mag
        c.append(max(prev + x, 1))
    return np.array(c, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------ rle_from_string
def test_from_string_equals_the_golden_vectors(cases):
    strs = [c["string"] for c in cases]
    hs, ws = [c["h"] for c in cases], [c["w"] for c in cases]
    cap = max(c["counts"].size for c in cases)
    got = from_strings(strs, hs, ws, cap)
    check_rows(got, strs, hs, ws, cap, "codec.npz")
    for i, c in enumerate(cases):                                   # and against the reference's own counts
        assert got[0][i] == c["counts"].size and np.array_equal(got[1][i, :c["counts"].size], c["counts"]), c["name"]
    r = list(rle_cases())
    strs, hs, ws = [c["string"] for c in r], [c["mask"].shape[0] for c in r], [c["mask"].shape[1] for c in r]
    cap = max(c["counts"].size for c in r)
    got = from_strings(strs, hs, ws, cap)
    check_rows(got, strs, hs, ws, cap, "rle.npz")
    assert not got[2].any()                                         # real masks: no flag
    for i, c in enumerate(r):
        assert np.array_equal(got[1][i, :c["counts"].size], c["counts"]), c["name"]


def test_from_string_carries_both_parity_chains_through_20000_tokens(ops):
    from maskrcnn_amd import image
    want = seeded_counts(np.random.default_rng(11), 20000)
    s = np_string(want)
    assert np.array_equal(image.rle_counts(s), want) and len(s) > 40000
    got = from_strings([s], [1], [1], 20000)
    assert got[0][0] == 20000 and np.array_equal(got[1][0], want) and got[2][0] == PIXEL_SUM
    # the op itself, through the packed tensors
    nr, cnt, st = ops.rle_from_string(dev(np.frombuffer(s, np.uint8).copy()), dev([0, len(s)], np.int64), dev([1], np.int32),
                                      dev([1], np.int32), capacity=20001)
    assert int(nr[0]) == 20000 and np.array_equal(cnt[0, :20000].cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("n", [1, 257])
def test_from_string_seeded_batches_with_empty_strings_and_an_offset_start(n):
    rng = np.random.default_rng(100 + n)
    strs = []
    for i in range(n):
        strs.append(b"" if (n > 1 and i % 5 == 1) else np_string(seeded_counts(rng, int(rng.integers(0, 76)))))   # <= 4 characters a run
    assert max(len(s) for s in strs) <= 300 and (n == 1 or min(len(s) for s in strs) == 0)
    hs, ws = [int(v) for v in rng.integers(1, 500, n)], [int(v) for v in rng.integers(1, 500, n)]
    check_rows(from_strings(strs, hs, ws, 80, prefix=b"\x00\xff/p0123"), strs, hs, ws, 80, f"n={n}")


def test_from_string_over_capacity_row_reports_its_count_and_is_untouched(cases):
    by = {c["name"]: c for c in cases}
    picks = [by["runs63_37"], by["runs1025_37"], by["runs64_37"], by["runs65_37"]]
    strs, hs, ws = [c["string"] for c in picks], [c["h"] for c in picks], [c["w"] for c in picks]
    got = from_strings(strs, hs, ws, 64)
    assert got[0].tolist() == [63, 1025, 64, 65]
    check_rows(got, strs, hs, ws, 64, "over capacity")


def test_from_string_refuses_malformed_strings_and_leaves_the_neighbours_intact(cases):
    good = {c["name"]: c for c in cases}["decode_5x7"]
    g, cap = good["string"], 40
    inner_empty = np_string([3, 0, 4, 28])            # flagged, written
    bad = [(g[:3] + b"/" + g[3:], 5, 7, BAD_BYTE), (g[:3] + b"p" + g[3:], 5, 7, BAD_BYTE), (g + b"P", 5, 7, OPEN_TOKEN),
           (b"PPPPPP0" + g, 5, 7, LONG_TOKEN), (g, 0, 7, BAD_SIZE), (g, 5, 16385, BAD_SIZE), (b"h", 5, 7, OPEN_TOKEN)]
    strs, hs, ws = [g], [5], [7]
    for s, h, w, _ in bad:
        strs += [s, g]
        hs += [h, 5]
        ws += [w, 7]
    strs += [inner_empty, g, g]
    hs += [5, 5, 6]                                   # the last: a wrong pixel sum, flagged and written
    ws += [7, 7, 7]
    num_runs, counts, status = from_strings(strs, hs, ws, cap)
    for k, (_, _, _, bit) in enumerate(bad):
        i = 1 + 2 * k
        assert num_runs[i] == -1 and status[i] & bit and (counts[i] == POISON).all(), (k, status[i])
        assert not status[i] & (EMPTY_RUN | PIXEL_SUM)
    n = len(strs)
    for i in [0] + [2 + 2 * k for k in range(len(bad))] + [n - 2]:
        assert num_runs[i] == good["counts"].size and status[i] == 0, i
        assert np.array_equal(counts[i, :num_runs[i]], good["counts"]) and (counts[i, num_runs[i]:] == POISON).all(), i
    assert num_runs[n - 3] == 4 and status[n - 3] == EMPTY_RUN and counts[n - 3, :4].tolist() == [3, 0, 4, 28]
    assert num_runs[n - 1] == good["counts"].size and status[n - 1] == PIXEL_SUM
    assert np.array_equal(counts[n - 1, :num_runs[n - 1]], good["counts"])


# ------------------------------------------------------------------------------------------------ rle_area_bbox
def test_area_bbox_equals_the_golden_vectors_on_one_table_of_mixed_sizes(ops, cases):
    rows = [c["counts"] for c in cases]
    cap = max(len(r) for r in rows)
    num_runs, counts = table(rows, cap, fill=7)                       # nothing past num_runs is read
    num_runs = torch.cat([num_runs, dev([-1, cap + 1], np.int32)])    # a refused row, a row over its capacity
    counts = torch.cat([counts, counts[:2]])
    hs = dev([c["h"] for c in cases] + [5, 5], np.int32)
    ws = dev([c["w"] for c in cases] + [7, 7], np.int32)
    areas, bboxes = ops.rle_area_bbox(num_runs, counts, hs, ws)
    assert areas.dtype == torch.int32 and bboxes.dtype == torch.int32 and tuple(bboxes.shape) == (len(cases) + 2, 4)
    areas, bboxes = areas.cpu().numpy(), bboxes.cpu().numpy()
    for i, c in enumerate(cases):
        assert areas[i] == c["area"] and bboxes[i].tolist() == c["bbox"], c["name"]
    assert areas[-2:].tolist() == [-1, -1] and (bboxes[-2:] == -1).all()
    names = [c["name"] for c in cases]
    for name in ("tokens0", "tokens1", "tokens2", "tokens3", "empty_5x7", "full_5x7", "corner_tl_6x5", "corner_br_6x5",
                 "cross_column_24x10", "row_1x9", "col_9x1", "runs63_37", "runs1025_37", "one_run_16384sq"):
        assert name in names


def test_area_bbox_equals_the_encoder_on_real_masks(ops):
    from maskrcnn_amd import cocoeval
    r = list(rle_cases())
    num_runs, counts = table([c["counts"] for c in r])
    areas, bboxes = ops.rle_area_bbox(num_runs, counts, dev([c["mask"].shape[0] for c in r], np.int32),
                                      dev([c["mask"].shape[1] for c in r], np.int32))
    for i, c in enumerate(r):
        assert int(areas[i]) == c["area"] and bboxes[i].tolist() == c["bbox"], c["name"]
        a, bb = cocoeval._rle_area_bbox(c["counts"], *c["mask"].shape)
        assert int(areas[i]) == a and bboxes[i].tolist() == [int(v) for v in bb], c["name"]


# ------------------------------------------------------------------------------------------------ rle_to_string
def test_to_string_equals_the_golden_strings_and_round_trips(ops, cases):
    rows = [c["counts"] for c in cases]
    cap = max(len(r) for r in rows)
    num_runs, counts = table(rows, cap, fill=9)
    num_runs = torch.cat([num_runs[:5], dev([-1, cap + 1], np.int32), num_runs[5:]])   # unusable rows: empty strings
    counts = torch.cat([counts[:5], counts[:2], counts[5:]])
    data, off = ops.rle_to_string(num_runs, counts)
    assert data.dtype == torch.uint8 and off.dtype == torch.int64 and off.numel() == len(cases) + 3
    data, off = data.cpu().numpy(), off.cpu().numpy()
    want = [c["string"] for c in cases[:5]] + [b"", b""] + [c["string"] for c in cases[5:]]
    assert off[0] == 0 and off[-1] == data.size == sum(len(s) for s in want)
    for i, s in enumerate(want):
        assert data[off[i]:off[i + 1]].tobytes() == s, i
    # back again: the table
    hs = dev([c["h"] for c in cases], np.int32)
    ws = dev([c["w"] for c in cases], np.int32)
    num_runs, counts = table(rows, cap)
    d2, o2 = ops.rle_to_string(num_runs, counts, total_bytes=int(off[-1]) + 10)         # a given size: no host read
    nr, cnt, st = ops.rle_from_string(d2, o2, hs, ws, capacity=cap)
    assert torch.equal(nr, num_runs)
    live = torch.arange(cap, device=DEV)[None, :] < nr[:, None]
    assert torch.equal(torch.where(live, cnt, torch.zeros_like(cnt)), counts)
    # the row counts round the 1024-thread scan of the row bytes: one row, a row a thread, and the first with two for some
    short = [c for c in cases if c["counts"].size <= 70]
    for n in (1, 1024, 1025):
        picks = [short[(5 * i + 3) % len(short)] for i in range(n)]
        data, off = ops.rle_to_string(*table([c["counts"] for c in picks], 70, fill=9))
        data, off = data.cpu().numpy(), off.cpu().numpy()
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(c["string"]) for c in picks])])), n
        assert data.tobytes() == b"".join(c["string"] for c in picks), n


def test_to_string_with_a_buffer_one_byte_short_reports_the_true_total_and_stays_inside(cases):
    from maskrcnn_amd import _lib
    picks = cases[10:30]
    num_runs, counts = table([c["counts"] for c in picks])
    n, total = len(picks), sum(len(c["string"]) for c in picks)
    buf = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    nbytes = int(_lib.lib.mrcnn_rle_to_string_workspace_bytes(n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib.mrcnn_rle_to_string(num_runs.data_ptr(), counts.data_ptr(), n, counts.size(1), buf.data_ptr(), total - 1,
                                            0, 0, off.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream))
    buf, off = buf.cpu().numpy(), off.cpu().numpy()
    assert off[n] == total and off[0] == 0
    last = len(picks[-1]["string"])
    assert last > 0 and (buf[total - last:] == 0xEE).all()             # the row that would cross the end is not written at all
    for i, c in enumerate(picks[:-1]):
        assert buf[off[i]:off[i + 1]].tobytes() == c["string"], c["name"]


def test_rle_masks_from_table_gives_the_encoder_s_dicts():
    """Every mask of rle.npz, every size group; then all 29-row masks (widths 1 .. 1021) as ONE table, so that rows of very
    different lengths sit at non-zero row offsets of the [N, 6*capacity] layout."""
    from maskrcnn_amd import image
    by_size = {}
    for c in rle_cases():
        by_size.setdefault(c["mask"].shape, []).append(c)
    assert sum(len(g) for g in by_size.values()) >= 40 and len(by_size) >= 30
    for size, group in by_size.items():
        dense = dev(np.stack([c["mask"] for c in group]).astype(np.uint8))
        enc = image.rle_masks(dense)
        made = image.rle_masks_from_table(size, enc.num_runs, enc.counts)
        assert made.to_coco() == enc.to_coco() == [{"size": list(size), "counts": c["string"]} for c in group], size
        assert torch.equal(made.areas, enc.areas) and torch.equal(made.bboxes, enc.bboxes), size
        assert torch.equal(made.string_bytes, enc.string_bytes) and made.strings.shape == (len(group), 6 * enc.capacity), size
        live = torch.arange(made.strings.size(1), device=DEV)[None, :] < made.string_bytes[:, None]
        assert torch.equal(made.strings[live], enc.strings[live]) and not made.strings[~live].any(), size
        assert torch.equal(made.decode(), dense), size
    # one table of many lengths: the strings are a property of the run list alone, so the size handed over is irrelevant to them
    rows = [c for c in rle_cases() if c["mask"].shape[0] == 29] + [c for c in rle_cases() if c["mask"].shape[0] != 29][:12]
    assert len(rows) >= 15 and len({len(c["string"]) for c in rows}) >= 6
    num_runs, counts = table([c["counts"] for c in rows], fill=5)
    made = image.rle_masks_from_table((29, 7), num_runs, counts)
    assert [d["counts"] for d in made.to_coco()] == [c["string"] for c in rows]
    assert made.string_bytes.tolist() == [len(c["string"]) for c in rows]


def test_rle_masks_from_table_with_unusable_rows():
    from maskrcnn_amd import image
    rows = [c for c in rle_cases() if c["mask"].shape == (60, 90)]
    num_runs, counts = table([c["counts"] for c in rows] * 2, fill=5)
    cap = counts.size(1)
    for bad in (-1, cap + 1):
        nr = num_runs.clone()
        nr[1] = bad
        made = image.rle_masks_from_table((60, 90), nr, counts)
        assert made.num_runs.tolist() == nr.tolist()
        assert made.string_bytes.tolist() == [len(rows[0]["string"]), 0, len(rows[0]["string"]), len(rows[1]["string"])]
        assert made.areas.tolist() == [rows[0]["area"], -1, rows[0]["area"], rows[1]["area"]]
        assert made.bboxes.tolist() == [rows[0]["bbox"], [-1] * 4, rows[0]["bbox"], rows[1]["bbox"]]
        assert not made.strings[1].any() and not made.decode()[1].any()
        for k in (0, 2, 3):
            assert made.strings[k, :made.string_bytes[k]].cpu().numpy().tobytes() == rows[k % 2]["string"]
        with pytest.raises(RuntimeError, match=r"masks \[1\]"):
            made.to_coco()


def test_to_string_rows_leaves_out_a_row_longer_than_the_stride(ops):
    rows = [c for c in rle_cases() if c["mask"].shape == (60, 90)]
    num_runs, counts = table([c["counts"] for c in rows])
    short, long_ = sorted(len(c["string"]) for c in rows)
    assert short < long_
    strings, nbytes = ops.rle_to_string_rows(num_runs, counts, row_stride=short)
    assert tuple(strings.shape) == (2, short) and sorted(nbytes.tolist()) == [0, short]
    for k, c in enumerate(rows):
        want = c["string"] if len(c["string"]) == short else bytes(short)
        assert strings[k].cpu().numpy().tobytes() == want


# ------------------------------------------------------------------------------------------------ rle_decode
@pytest.mark.parametrize("size", [(1, 1), (1, 9), (9, 1), (5, 7), (37, 53), (64, 61), (65, 64), (33, 130)])
def test_decode_equals_the_golden_bits_into_a_strided_poisoned_buffer(ops, cases, size):
    from maskrcnn_amd import image
    h, w = size
    group = [c for c in cases if c["name"].startswith("decode_") and (c["h"], c["w"]) == size]
    assert len(group) == 4
    for n in (1, 3):
        picks = group[:n] if n == 3 else group[1:2]
        num_runs, counts = table([c["counts"] for c in picks], fill=3)
        whole = torch.full((n + 1, h + 3, w + 6), 0xCC, dtype=torch.uint8, device=DEV)
        out = whole[:n, 1:h + 1, 5:w + 5]                              # image and row strides of a view, an odd start
        assert ops.rle_decode(num_runs, counts, h, w, out=out) is out
        got = whole.cpu().numpy()
        for i, c in enumerate(picks):
            assert np.array_equal(got[i, 1:h + 1, 5:w + 5], c["mask"].astype(np.uint8)), c["name"]
            assert np.array_equal(c["mask"], image.rle_decode(c["counts"].tolist(), size=size)), c["name"]
        got[:n, 1:h + 1, 5:w + 5] = 0xCC
        assert (got == 0xCC).all()                                     # nothing outside
    num_runs, counts = table([c["counts"] for c in group])
    fresh = ops.rle_decode(num_runs, counts, h, w)
    assert fresh.dtype == torch.uint8 and tuple(fresh.shape) == (4, h, w)
    enc = ops.rle_encode(fresh, capacity=counts.size(1))              # and back: the table
    assert torch.equal(enc[0], num_runs)
    for i, c in enumerate(group):
        assert np.array_equal(enc[1][i, :c["counts"].size].cpu().numpy().view(np.uint32), c["counts"]), c["name"]


def test_decode_clips_long_rows_zero_fills_short_ones_and_unusable_rows(ops):
    rows = [[3, 100], [2, 1], [1, 1, 1, 1, 1, 1], [0, 6], [4, 0, 0, 1, 1]]
    num_runs, counts = table(rows, capacity=6, fill=1)
    num_runs = torch.cat([num_runs, dev([-1, 7], np.int32)])
    counts = torch.cat([counts, counts[3:5]])
    out = torch.full((7, 2, 3), 0xCC, dtype=torch.uint8, device=DEV)
    got = ops.rle_decode(num_runs, counts, 2, 3, out=out).cpu().numpy()
    col = lambda flat: np.array(flat, np.uint8).reshape(3, 2).T       # column-major pixels
    assert np.array_equal(got[0], col([0, 0, 0, 1, 1, 1]))            # clipped at h*w
    assert np.array_equal(got[1], col([0, 0, 1, 0, 0, 0]))            # pixels the runs do not reach are 0
    assert np.array_equal(got[2], col([0, 1, 0, 1, 0, 1]))
    assert np.array_equal(got[3], col([1, 1, 1, 1, 1, 1]))
    assert np.array_equal(got[4], col([0, 0, 0, 0, 1, 0]))            # empty runs in the middle: on, off, then on for one
    assert not got[5:].any()


def test_decode_inverts_the_encoder_on_two_large_masks(ops):
    from maskrcnn_amd import image
    g = torch.Generator(device="cpu").manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(1200, device=DEV), torch.arange(1920, device=DEV), indexing="ij")
    masks = torch.zeros(2, 1200, 1920, dtype=torch.bool, device=DEV)
    for i in range(2):
        for cy, cx, r in torch.rand(5, 3, generator=g).tolist():
            masks[i] |= (yy - cy * 1200) ** 2 + (xx - cx * 1920) ** 2 <= (40 + 300 * r) ** 2
    masks[0, 0, 0] = True
    masks[1, -1, -1] = True
    masks = masks.view(torch.uint8)
    enc = image.rle_masks(masks)
    assert int(enc.num_runs.max()) <= enc.capacity and int(enc.num_runs.min()) > 1000
    assert torch.equal(ops.rle_decode(enc.num_runs, enc.counts, 1200, 1920), masks) and torch.equal(enc.decode(), masks)


# ------------------------------------------------------------------------------------------------ image / cocoeval
def test_rle_table_on_the_device_merges_strings_and_count_lists_and_keeps_its_errors():
    from maskrcnn_amd import image
    r = [c for c in rle_cases() if c["mask"].shape == (29, 13) or c["mask"].shape == (60, 90)]
    same = [c for c in r if c["mask"].shape == (60, 90)]
    assert len(same) >= 2
    objs = [{"size": [60, 90], "counts": same[0]["string"]}, same[1]["counts"].tolist(), same[1]["string"].decode("ascii"),
            {"size": [60, 90], "counts": same[0]["counts"].tolist()}, same[0]["string"]]
    num_runs, counts = image.rle_table(objs, (60, 90), DEV)
    ref_runs, ref_counts = image.rle_table(objs, (60, 90), "cpu")
    assert torch.equal(num_runs.cpu(), ref_runs) and torch.equal(counts.cpu(), ref_counts)
    wide = image.rle_table(objs, (60, 90), DEV, capacity=counts.size(1) + 5)
    assert torch.equal(wide[1].cpu(), image.rle_table(objs, (60, 90), "cpu", capacity=counts.size(1) + 5)[1])
    assert torch.equal(image.rle_decode_masks(objs, (60, 90), DEV)[0].cpu(), torch.from_numpy(same[0]["mask"].astype(np.uint8)))
    for bad, match in ((objs[:4] + [{"size": [60, 91], "counts": same[0]["string"]}], "mask 4 is"),
                       (objs[:2] + [np_string([10, 20])], "the runs of mask 2 cover 30 pixels, the mask has 60 x 90"),
                       (objs[:1] + [np_string([5000, 0, 400])], "mask 1 has an empty run after the first one"),
                       ([same[0]["string"] + b"P"], "mask 0 has a compressed string that ends inside a run"),
                       ([same[0]["string"], b"0/"], "mask 1 has a character outside"),
                       ([b"PPPPPPP0"], "mask 0 has a run of more than 6 characters")):
        with pytest.raises(ValueError, match=match):
            image.rle_table(bad, (60, 90), DEV)
    with pytest.raises(ValueError, match="capacity 2 is less than the longest mask's"):
        image.rle_table(objs, (60, 90), DEV, capacity=2)


def test_the_lowest_bad_entry_is_named_whatever_its_kind():
    """A malformed string (found by the kernel's status) and a bad count list (found on the host) in one list: the error is the
    lower index's, in either order, through rle_table and through evaluate's ground-truth table."""
    from maskrcnn_amd import cocoeval, image
    good = [c for c in rle_cases() if c["mask"].shape == (60, 90)][0]["string"]
    open_string, short_list = good + b"P", [10, 20]
    for bad, match in (([open_string, short_list], "mask 1 has a compressed string that ends inside a run"),
                       ([short_list, open_string], "the runs of mask 1 cover 30 pixels, the mask has 60 x 90")):
        with pytest.raises(ValueError, match=match):
            image.rle_table([good] + bad, (60, 90), DEV)
        seg = lambda c: {"size": [60, 90], "counts": c.decode("ascii") if isinstance(c, bytes) else c}
        gt = dict(images=[dict(id=1, height=60, width=90), dict(id=2, height=60, width=90)], categories=[dict(id=1)],
                  annotations=[dict(id=k + 1, image_id=min(k + 1, 2), category_id=1, iscrowd=0, area=100.0, bbox=[0.0, 0.0, 10.0, 10.0],
                                    segmentation=seg(c)) for k, c in enumerate([good] + bad)])
        results = [dict(image_id=1, category_id=1, score=0.5, segmentation=seg(good))]
        with pytest.raises(ValueError, match=match):
            cocoeval.evaluate(gt, results, "segm")


def strip_bbox(results):
    return [{k: v for k, v in r.items() if k != "bbox"} for r in results]


def same_evaluation(a, b):
    assert np.array_equal(a.stats, b.stats) and np.array_equal(a.precision, b.precision) and np.array_equal(a.recall, b.recall)
    assert np.array_equal(a.scores, b.scores) and a.summary() == b.summary()
    assert a.ious.keys() == b.ious.keys()
    for key in a.ious:
        assert np.array_equal(np.asarray(a.ious[key]), np.asarray(b.ious[key])), key
    assert len(a.eval_imgs) == len(b.eval_imgs) and all(same_eval_img(x, y) for x, y in zip(a.eval_imgs, b.eval_imgs))


def test_load_results_on_the_device_gives_the_same_areas_and_boxes():
    from maskrcnn_amd import cocoeval
    _, results = golden_inputs()
    results = strip_bbox(results)
    host, gpu = cocoeval.load_results(results, "segm"), cocoeval.load_results(results, "segm", device=DEV)
    assert len(host) == len(gpu) == len(results) and isinstance(gpu, list)
    for a, b in zip(host, gpu):
        assert type(b["area"]) is np.uint32 and b["area"] == a["area"]
        assert isinstance(b["bbox"], np.ndarray) and b["bbox"].dtype == a["bbox"].dtype and np.array_equal(a["bbox"], b["bbox"])
        assert {k: v for k, v in a.items() if k not in ("area", "bbox")} == {k: v for k, v in b.items() if k not in ("area", "bbox")}
    bad = json.loads(json.dumps(results[:3]))
    bad[1]["segmentation"]["counts"] += "P"
    with pytest.raises(ValueError, match="result 1: the segmentation has a compressed string that ends inside a run"):
        cocoeval.load_results(bad, "segm", device=DEV)


def test_evaluate_decodes_strings_on_the_device_and_equals_the_host_route(monkeypatch):
    from maskrcnn_amd import cocoeval, image
    z = load_golden("cocoeval")
    gt, results = golden_inputs()
    assert all(isinstance(r["segmentation"]["counts"], str) for r in results)
    host = [cocoeval._evaluate(gt, res, "segm", DEV, "error", "host") for res in (results, strip_bbox(results))]
    assert np.array_equal(host[0].stats, z["segm_stats"])
    for res, want in zip((results, strip_bbox(results)), host):
        same_evaluation(cocoeval.evaluate(gt, res, "segm"), want)
    # the per-character loop is gone: rle_counts may no longer see a string
    real = image.rle_counts

    def no_strings(obj):
        c = obj["counts"] if isinstance(obj, dict) else obj
        assert not isinstance(c, (str, bytes, bytearray)), "image.rle_counts was handed a compressed string"
        return real(obj)

    monkeypatch.setattr(image, "rle_counts", no_strings)
    for res, want in zip((results, strip_bbox(results)), host):
        same_evaluation(cocoeval.evaluate(gt, res, "segm"), want)


def test_ann_to_rle_compress_writes_the_strings_of_the_uncompressed_result():
    from maskrcnn_amd import cocoeval, image
    from test_poly_host import eval_inputs
    gt, _ = eval_inputs()
    plain, packed = cocoeval.ann_to_rle(gt, DEV), cocoeval.ann_to_rle(gt, DEV, compress=True)
    polys = 0
    for src, a, b in zip(gt["annotations"], plain["annotations"], packed["annotations"]):
        if isinstance(src["segmentation"], list):
            polys += 1
            assert isinstance(b["segmentation"]["counts"], bytes) and b["segmentation"]["size"] == a["segmentation"]["size"]
            assert image.rle_counts(b["segmentation"]).tolist() == a["segmentation"]["counts"]
            assert b["segmentation"]["counts"] == np_string(a["segmentation"]["counts"])
        else:
            assert b["segmentation"] == src["segmentation"]
    assert polys > 3


COUNTED = ("rle_from_string", "rle_area_bbox", "rle_from_poly", "rle_merge", "rle_iou", "bbox_iou", "coco_match", "rle_encode")


def test_library_calls_of_one_evaluation_are_counted(ops, monkeypatch):
    """How many times each library entry point runs in one evaluate / load_results / ann_to_rle call. The numbers were recorded
    on the commit before the table building of image.rle_table and cocoeval.evaluate was put in one place, with this test; the
    host code around the kernels may be rearranged, the device work of a call may not."""
    from maskrcnn_amd import cocoeval
    from test_poly_host import eval_inputs
    calls = dict.fromkeys(COUNTED, 0)

    def counting(name, real):
        def wrapper(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return wrapper

    for name in COUNTED:
        monkeypatch.setattr(ops, name, counting(name, getattr(ops, name)))

    def count(fn):
        for name in COUNTED:
            calls[name] = 0
        fn()
        return {k: v for k, v in calls.items() if v}

    gt, results = golden_inputs()
    poly_gt, poly_results = eval_inputs()
    assert count(lambda: cocoeval.evaluate(gt, results, "segm")) == dict(rle_from_string=2, rle_iou=1, coco_match=1)
    assert count(lambda: cocoeval.evaluate(gt, strip_bbox(results), "segm")) == \
        dict(rle_from_string=2, rle_area_bbox=1, rle_iou=1, coco_match=1)
    # poly.npz's ground truth holds polygons and count lists, no compressed string: the one decode is the results'
    assert count(lambda: cocoeval.evaluate(poly_gt, poly_results, "segm", polygons="rasterize")) == \
        dict(rle_from_string=1, rle_from_poly=1, rle_merge=1, rle_iou=1, coco_match=1)
    assert count(lambda: cocoeval.load_results(strip_bbox(results), "segm", device=DEV)) == dict(rle_from_string=1, rle_area_bbox=1)
    assert count(lambda: cocoeval.ann_to_rle(poly_gt, DEV)) == dict(rle_from_poly=1, rle_merge=1)
