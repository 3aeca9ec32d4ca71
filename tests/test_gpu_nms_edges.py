"""GPU tests (-m gpu) of csrc/nms.hip and csrc/nms_general.hip on the constructed cases of tests/nms_cases.py: chains that make
the greedy resolution 64 deep, chain neighbours whose IoU is exactly the threshold, dead boxes whose victims sit a known number of
chunks later, fp64 boxes against the float threshold, every plan of the launcher, class ids, segment counts with poisoned rows
behind them, non-finite scores and coordinates, thresholds outside (0, 1) and strided views. The expectation is the closed form
(integer logic on the chains) where a case has one and the numpy restatement nms_stepwise otherwise;
tests/test_nms_cases_host.py proves both against the C oracle without a GPU.

Every kernel is called through the C ABI into guarded buffers: keep, counts and the workspace (exactly *_workspace_bytes long) sit
between bands of a fill value that must be intact after the call, the input must be bit-identical afterwards, and a second call
must give the same bits. The file runs once more in a child pytest on the schedule-fuzz library."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nms_cases as nc
from nms_cases import f32, f64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_LIB = os.path.join(ROOT, "maskrcnn_amd", "csrc", "build", "variants", "sync_fuzz", "libmaskrcnn_hip.so")
BAND = 4096   # elements on either side of an output (a multiple of the 256 bytes nms_general's workspace is aligned to)
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
CASES = nc.all_cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import maskrcnn_amd  # noqa: F401  must load libmaskrcnn_hip.so or fail loudly
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------ plumbing
class _Out:
    """An output tensor of `shape` in the middle of a buffer filled with `fill`."""

    def __init__(self, shape, dtype, dev, fill=7):
        self.n, self.fill = int(np.prod(shape, dtype=np.int64)), fill
        self.buf = torch.full((self.n + 2 * BAND,), fill, dtype=dtype, device=dev)
        self.t = self.buf[BAND:BAND + self.n].view(*shape)

    @property
    def ptr(self):
        return self.buf.data_ptr() + BAND * self.buf.element_size()

    def intact(self):
        return bool((self.buf[:BAND] == self.fill).all()) and bool((self.buf[BAND + self.n:] == self.fill).all())


def _raw(t):
    """The bits of a tensor's whole buffer (the view's base)."""
    base = t if t._base is None else t._base
    return base.contiguous().view(-1).view(torch.int32 if base.element_size() == 4 else torch.int64).clone()


def _twice(call, outs, inputs):
    """Two identical C-ABI calls: bands intact, inputs untouched, the same bits both times. → the outputs of the first (host)."""
    from maskrcnn_amd._lib import check
    before = [_raw(t) for t in inputs]
    got = []
    for _ in range(2):
        for o in outs[:2]:
            o.t.fill_(-77)
        check(call())
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            assert o.intact(), f"output {i} written outside its {o.n} elements"
        for t, b in zip(inputs, before):
            assert torch.equal(_raw(t), b), "an input was written"
        got.append([o.t.cpu().numpy().copy() for o in outs[:2]])
    assert all(np.array_equal(a, b) for a, b in zip(*got)), "the second call gave other bits"
    return got[0]


def _batched(dets, thr, use_ws, dev, counts=None, cls=None):
    """mrcnn_nms_batched_f32 on dets [S, N, >= 5] (a device view with any strides). → keep [S, N], counts [S] (numpy)."""
    from maskrcnn_amd._lib import lib
    s, n = dets.shape[:2]
    keep, cnt = _Out((s, n), I64, dev), _Out((s,), I32, dev)
    nbytes = int(lib.mrcnn_nms_workspace_bytes(s, n)) if use_ws else 0
    assert nbytes <= 33 << 20
    ws = _Out((nbytes,), U8, dev, fill=0xA5) if use_ws else None
    ins = [t for t in (dets, counts, cls) if t is not None]
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: lib.mrcnn_nms_batched_f32(dets.data_ptr(), s, n, *dets.stride(), None if counts is None else counts.data_ptr(),
                                             None if cls is None else cls.data_ptr(), float(thr), keep.ptr, cnt.ptr,
                                             ws.ptr if use_ws else None, nbytes, stream)
    return _twice(call, [keep, cnt] + ([ws] if use_ws else []), ins)


def _general(dets, thr, dev):
    """mrcnn_nms_general on dets [N, >= 5] float32 / float64 (a device view with any strides). → keep [N], count [1] (numpy)."""
    from maskrcnn_amd._lib import lib
    n, dt = dets.size(0), {torch.float32: 0, torch.float64: 1}[dets.dtype]
    keep, cnt = _Out((n,), I64, dev), _Out((1,), I64, dev)
    nbytes = int(lib.mrcnn_nms_general_workspace_bytes(n, dt))
    ws = _Out((nbytes,), U8, dev, fill=0xA5)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: lib.mrcnn_nms_general(dets.data_ptr(), dt, n, *dets.stride(), float(thr), keep.ptr, cnt.ptr, ws.ptr, nbytes,
                                         stream)
    return _twice(call, [keep, cnt, ws], [dets])


def _assert_keep(keep, count, want, tag):
    assert int(count) == want.size, (tag, int(count), want.size)
    assert np.array_equal(keep[:want.size], want), tag
    assert (keep[want.size:] == -1).all(), tag


@functools.lru_cache(maxsize=None)
def _want(name, dtype):
    """Computed once per case and type, shared by the tests, never written to."""
    case = CASES[name]
    want = nc.expected_keep(case, dtype)
    if want is None:
        want = nc.nms_stepwise(case.dets, case.thr, case.class_ids, dtype)
    want.setflags(write=False)
    return want


def _run_path(case, path, dev):
    if path in ("lds", "ws"):
        d = torch.from_numpy(case.dets).float().to(dev).unsqueeze(0)
        cls = None if case.class_ids is None else torch.from_numpy(case.class_ids).to(dev)
        keep, cnt = _batched(d, case.thr, path == "ws", dev, cls=cls)
        return keep[0], cnt[0]
    d = torch.from_numpy(case.dets).to(torch.float32 if path == "gen32" else torch.float64).to(dev)
    keep, cnt = _general(d, case.thr, dev)
    return keep, cnt[0]


# ------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", list(CASES))
def test_case_on_every_path_that_takes_it(dev, name):
    """Kept indices equal the expectation exactly, the tail is -1, the count is equal — on the LDS kernel, the workspace path and
    nms_general in fp32 and fp64, whichever take the case — and the LDS and workspace paths give identical outputs."""
    from maskrcnn_amd import ops
    case = CASES[name]
    got = {}
    for path in case.paths:
        if path in ("lds", "ws"):
            assert ops.nms_plan(case.n, path == "ws").path == ("workspace" if path == "ws" else "lds")
        keep, cnt = got[path] = _run_path(case, path, dev)
        _assert_keep(keep, cnt, _want(name, f64 if path == "gen64" else f32), (name, path))
    if "lds" in got and "ws" in got:
        assert np.array_equal(got["lds"][0], got["ws"][0]) and got["lds"][1] == got["ws"][1]


def test_fp64_boxes_meet_the_float_threshold_converted_to_double(dev):
    """(13, 7) chains at 0.3: every neighbour IoU is 3/10. fp32: fl32(3/10) == 0.3f suppresses, alternate chain elements go.
    fp64: 0.3 < (double)0.3f, every box stays. The same boxes, the same call, only the type differs."""
    for n in (321, 1089):
        case = CASES[f"composite-n{n}-thr0.3"]
        keep32, c32 = _run_path(case, "gen32", dev)
        keep64, c64 = _run_path(case, "gen64", dev)
        assert c64 == n and np.array_equal(keep64, np.arange(n))
        assert c32 == nc.expected_keep(case, f32).size < n


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if c.class_ids is None])
def test_single_segment_cases_through_the_python_entry_points(dev, name):
    """maskrcnn.nms (dispatches on n and dtype), ops.nms_batched (both paths) and ops.nms_general on the same cases."""
    import maskrcnn
    from maskrcnn_amd import ops
    case = CASES[name]
    d32 = torch.from_numpy(case.dets).float().to(dev)
    assert np.array_equal(maskrcnn.nms(d32, case.thr).cpu().numpy(), _want(name, f32)), name
    for path in case.paths:
        if path in ("lds", "ws"):
            keep, cnt = ops.nms_batched(d32.unsqueeze(0), case.thr, use_workspace=path == "ws")
            _assert_keep(keep[0].cpu().numpy(), cnt[0], _want(name, f32), (name, path))
        else:
            dtype = f64 if path == "gen64" else f32
            d = d32 if path == "gen32" else torch.from_numpy(case.dets).to(dev)
            keep, cnt = ops.nms_general(d, case.thr)
            _assert_keep(keep.cpu().numpy(), cnt[0], _want(name, dtype), (name, path))
            if path == "gen64":
                assert np.array_equal(maskrcnn.nms(d, case.thr).cpu().numpy(), _want(name, f64)), name


# ------------------------------------------------------------------------------------------------------ segments
@pytest.mark.parametrize("n_max", [130, 300, 1089])
def test_segments_counts_and_poisoned_rows_behind_them(dev, n_max):
    """S = 6, counts n_max, 0, 1, 64, 65, n_max - 1; the rows behind a count hold NaN / +inf scores, NaN / infinite coordinates
    and higher-scored copies of the segment's own boxes. Each segment equals its first `count` rows alone; segment s of the batch
    equals segment s as a batch of one, bit for bit; counts of -3 and n_max + 7 are clamped to 0 and n_max."""
    seg = nc.segments_case(n_max)
    want_keep, want_cnt = seg.expected()
    d = torch.from_numpy(seg.dets).float().to(dev)
    counts = torch.from_numpy(seg.counts).to(dev)
    for use_ws in (False, True):
        keep, cnt = _batched(d, seg.thr, use_ws, dev, counts=counts)
        assert np.array_equal(cnt, want_cnt) and np.array_equal(keep, want_keep), (n_max, use_ws)
        for s in range(6):
            k1, c1 = _batched(d[s:s + 1], seg.thr, use_ws, dev, counts=counts[s:s + 1])
            assert np.array_equal(k1[0], keep[s]) and c1[0] == cnt[s], (n_max, use_ws, s)
        clamped = counts.clone()
        clamped[0], clamped[1] = n_max + 7, -3
        keep, cnt = _batched(d, seg.thr, use_ws, dev, counts=clamped)
        assert np.array_equal(cnt, want_cnt) and np.array_equal(keep, want_keep), (n_max, use_ws, "clamp")


# ------------------------------------------------------------------------------------------------------ strides
def test_strided_views(dev):
    """dets as views: col_stride != 1 (a [S, 7, N] buffer transposed), row_stride 9 with a column offset, a seg_stride that is
    not N rows (every other slice of an [N, 3, 5] buffer); everything outside the views is NaN. Segment 0 is the n = 321
    composite at 0.5, segment 1 the (13, 7) composite, whose neighbours (3/10) stay below 0.5: every box kept."""
    n = 321
    a, b = CASES["composite-n321-thr0.5"], CASES["composite-n321-thr0.3"]
    want = [_want(a.name, f32), np.arange(n)]
    both = torch.from_numpy(np.stack([a.dets, b.dets])).float().to(dev)                   # [2, n, 5]
    nan = float("nan")
    cols = torch.full((2, 7, n), nan, device=dev)
    cols[:, 1:6] = both.transpose(1, 2)
    rows = torch.full((2, n, 9), nan, device=dev)
    rows[:, :, 2:7] = both
    segs = torch.full((n, 3, 5), nan, device=dev)
    segs[:, 0], segs[:, 2] = both[0], both[1]
    views = {"col_stride": cols.transpose(1, 2)[:, :, 1:6], "row_stride": rows[:, :, 2:7], "seg_stride": segs.permute(1, 0, 2)[::2]}
    assert views["col_stride"].stride() == (7 * n, 1, n) and views["row_stride"].stride() == (9 * n, 9, 1)
    assert views["seg_stride"].stride() == (10, 15, 1)
    for tag, v in views.items():
        assert torch.equal(v, both)
        for use_ws in (False, True):
            keep, cnt = _batched(v, 0.5, use_ws, dev)
            for s in range(2):
                _assert_keep(keep[s], cnt[s], want[s], (tag, use_ws, s))
        for dtype in (torch.float32, torch.float64):
            v2 = (v if dtype == torch.float32 else {"col_stride": cols.double().transpose(1, 2)[:, :, 1:6],
                                                    "row_stride": rows.double()[:, :, 2:7],
                                                    "seg_stride": segs.double().permute(1, 0, 2)[::2]}[tag])
            for s in range(2):
                keep, cnt = _general(v2[s], 0.5, dev)
                _assert_keep(keep, cnt[0], want[s], (tag, dtype, s))


# --------------------------------------------------------------------------------------------------------- schedule fuzzing
# The child's time limit: four times the wall time measured on the fuzzed library, rounded up to 30 s: 5.7 s (147 tests; 3.7 s of
# it inside pytest, the rest start-up), so 22.8 s -> 30 s.
FUZZ_TIMEOUT = 30


@pytest.mark.skipif(os.environ.get("MRCNN_SYNC_FUZZ_CHILD") == "1", reason="this IS the fuzzed child run")
def test_this_file_passes_under_schedule_fuzzing():
    """nms_kernel hands the chunk's row masks and survivor word from wave to wave through LDS between barriers, nms_scan_kernel its
    column words and keep flags; on that build every wave sleeps a random time behind each barrier, and a hand-off that the
    barrier does not order fails its exact comparison there."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_nms_edges.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=FUZZ_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
