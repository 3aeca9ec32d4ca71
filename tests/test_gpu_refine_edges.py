"""GPU tests (-m gpu) of the refine-stage kernels where they compare, branch and index: non-finite values, ties, and sizes
that leave every tile, wave and vector loop ragged.

    csrc/misc.hip    rpn_scores_deltas, proposal_decode, detection_decode
    csrc/select.hip  topk_desc, proposal_select, detection_select
    csrc/crop.hip    the side paths of the pyramid RoIAlign (roi_batch, roi_counts, layouts, pool 1) and crop_backward

References are float64 numpy / torch restatements of the formulas in include/maskrcnn_hip.h, written here; oracle.rpn_refine and
oracle.mrn_refine serve at stage level. Every kernel is called through the C ABI into guarded buffers (a band of a fill value on
either side of each output, checked after the call), so a store outside the documented output fails the test that made it."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAND = 4096   # elements on either side of an output
F32, I32, I64 = torch.float32, torch.int32, torch.int64
STD = [0.1, 0.1, 0.2, 0.2]


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
        return self.t.data_ptr() if self.n else self.buf.data_ptr() + BAND * self.buf.element_size()

    def intact(self):
        return bool((self.buf[:BAND] == self.fill).all()) and bool((self.buf[BAND + self.n:] == self.fill).all())


def _run(fn, args, outs):
    """One C-ABI call on the current stream; every guarded output's bands must be untouched afterwards."""
    from maskrcnn_amd._lib import check
    check(fn(*args, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert o.intact(), f"{fn.__name__}: output {i} written outside its {o.n} elements"


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _bits_equal(a, b):
    """Bit for bit: NaN payloads and the sign of a zero included."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _neg_nan():
    """The NaN x86 produces for inf - inf: sign bit set (0xFFC00000)."""
    return float(np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0])


def _arr(ctype, values):
    return (ctype * len(values))(*values)


# =========================================================================================== rpn_scores_deltas
def _rpn(heads, hs, ws, modes, bias, batch, dev):
    from maskrcnn_amd._lib import c_i32, c_vp, lib
    a = 3 * sum(h * w for h, w in zip(hs, ws))
    scores, deltas = _Out((batch, a), F32, dev), _Out((batch, a, 4), F32, dev)
    _run(lib.mrcnn_rpn_scores_deltas_v2_f32,
         (_arr(c_vp, [t.data_ptr() for t in heads]), _arr(c_i32, hs), _arr(c_i32, ws), _arr(c_i32, modes),
          None if bias is None else bias.data_ptr(), batch, scores.ptr, deltas.ptr), (scores, deltas))
    return scores.t.cpu(), deltas.t.cpu()


RPN_SIZES = [(17, 13), (9, 7), (5, 3), (2, 1), (1, 1)]
# l1 - l0 of the planted logit pairs: the issue's set, plus a sweep that puts scores into [1e-30, 1e-6]
RPN_DIFFS = [0.0] + [s * v for v in (1e-3, 20.0, 88.0, 104.0, 200.0) for s in (1.0, -1.0)] + \
            [float(v) for v in np.linspace(-69.0, -14.0, 56)]


def _rpn_edge_heads(batch, seed):
    g = torch.Generator().manual_seed(seed)
    heads = [torch.randn(batch, h, w, 18, generator=g) * 2 for h, w in RPN_SIZES]
    first = np.cumsum([0] + [3 * h * w for h, w in RPN_SIZES])
    pairs = [(-d / 2, d / 2) for d in RPN_DIFFS] + [(1e30, 1e30)]
    # the first and the last anchor of every level, then the anchors after the first one of level 0
    slots = [int(a) for l in range(5) for a in (first[l], first[l + 1] - 1)]
    slots = list(dict.fromkeys(slots))
    slots += [a for a in range(1, 200) if a not in slots][:len(pairs) - len(slots)]
    assert len(slots) == len(pairs)
    for b in range(batch):
        for i, a in enumerate(slots):
            l0, l1 = pairs[(i + 7 * b) % len(pairs)]          # another pair on each boundary in each image
            lvl = int(np.searchsorted(first, a, side="right") - 1)
            pix, r = divmod(a - int(first[lvl]), 3)
            row = heads[lvl][b].view(-1, 18)[pix]
            row[2 * r], row[2 * r + 1] = l0, l1
    return heads


def _rpn_reference(heads):
    batch = heads[0].size(0)
    logits = torch.cat([t[..., :6].reshape(batch, -1, 2) for t in heads], 1)      # anchor = first(l) + (y*W + x)*3 + ratio
    deltas = torch.cat([t[..., 6:].reshape(batch, -1, 4) for t in heads], 1)
    l64 = logits.double().numpy()
    with np.errstate(over="ignore"):
        want = 1.0 / (1.0 + np.exp(l64[..., 0] - l64[..., 1]))
    return logits, deltas, want


def _softmax_rel_error(logits, want):
    """Worst relative error of torch's CPU fp32 softmax against float64 where the score lies in [1e-30, 1e-6]."""
    cpu = torch.softmax(logits, dim=2)[..., 1].double().numpy()
    m = (want >= 1e-30) & (want <= 1e-6)
    assert m.sum() >= 40
    return float((np.abs(cpu - want)[m] / want[m]).max()), m


@pytest.mark.parametrize("batch", [1, 3])
def test_rpn_scores_deltas_odd_levels_and_extreme_logit_pairs(dev, batch):
    """Levels (17,13) (9,7) (5,3) (2,1) (1,1), logit pairs with l1 - l0 in {0, +-1e-3, +-20, +-88, +-104, +-200}, (1e30, 1e30)
    and a sweep over [-69, -14] planted on the first and last anchor of every level and behind them. Scores against float64
    1/(1+exp(l0-l1)): 2e-7 absolute (the bound of test_rpn_scores_deltas_and_proposal_decode), and for scores in
    [1e-30, 1e-6] relative within 4x the worst relative error of torch's CPU fp32 softmax on the same inputs, which is
    measured in the test (7.2e-8 at either batch size, about one ulp; the two expf differ by ulps, hence the factor). Deltas
    bit for bit."""
    heads = _rpn_edge_heads(batch, 310 + batch)
    logits, want_deltas, want = _rpn_reference(heads)
    hs, ws = [h for h, _ in RPN_SIZES], [w for _, w in RPN_SIZES]
    scores, deltas = _rpn([t.to(dev) for t in heads], hs, ws, [0] * 5, None, batch, dev)
    assert _bits_equal(deltas, want_deltas)
    got = scores.double().numpy()
    assert not np.isnan(got).any()
    err = np.abs(got - want).max()
    cpu_rel, m = _softmax_rel_error(logits, want)
    rel = float((np.abs(got - want)[m] / want[m]).max())
    print(f"batch {batch}: max abs err {err:.3e}; scores in [1e-30, 1e-6]: {int(m.sum())}, worst relative error "
          f"{rel:.3e} (torch CPU fp32 softmax: {cpu_rel:.3e})")
    assert err <= 2e-7
    assert rel <= 4 * cpu_rel


def _head_rows(mode, batch, h, w):
    """Row of pixel (b, y, x) in a head_part tensor, by the formulas of include/maskrcnn_hip.h
    (mrcnn_conv3x3_winograd_heads_f32, mrcnn_conv3x3_winograd4_heads_f32, mrcnn_rpn_scores_deltas_v2_f32)."""
    b, y, x = np.meshgrid(np.arange(batch), np.arange(h), np.arange(w), indexing="ij")
    cdiv = lambda p, q: -(-p // q)
    if mode == 1:
        return ((b * (h // 2) + y // 2) * (w // 2) + x // 2) * 4 + (y & 1) * 2 + (x & 1)
    if mode == 2:
        mt = (b * cdiv(h, 16) + y // 16) * cdiv(w, 16) + x // 16
        return mt * 256 + ((y // 2 & 7) * 8 + (x // 2 & 7)) * 4 + (y & 1) * 2 + (x & 1)
    if mode == 3:
        mt = (b * cdiv(h, 16) + y // 16) * cdiv(w, 32) + x // 32
        return mt * 512 + ((y // 4 & 3) * 8 + (x // 4 & 7)) * 16 + (y & 3) * 4 + (x & 3)
    assert mode == 4
    return (b * h + y) * w + x


def test_rpn_scores_deltas_head_sum_forms_equal_the_nhwc_form(dev):
    """Input forms 1-4 (the head sums of the Winograd / pipelined fp16 convs, bias not yet added), built on the host from
    known [B,H,W,18] planes by the header's row formulas, at sizes where the tile counts are ragged (form 2: H/2 = 11, W/2 = 13;
    form 3: H/4 = 5, W/4 = 11; form 1: 30 positions in a 64-position tile), batch 2, every unused row and column NaN. The
    result must equal form 0 on (p0 + p1) + bias computed in fp32, bit for bit, and hold no NaN."""
    from maskrcnn_amd._lib import lib
    g = torch.Generator().manual_seed(77)
    batch = 2
    levels = [(22, 26, 2), (20, 44, 3), (6, 10, 1), (3, 5, 4), (1, 1, 0)]
    bias = torch.randn(18, generator=g)
    parts, nhwc = [], []
    for h, w, mode in levels:
        p0 = torch.randn(batch, h, w, 18, generator=g) * 2
        if mode == 0:
            parts.append(p0)
            nhwc.append(p0)
            continue
        total = torch.randn(batch, h, w, 18, generator=g) * 2
        p1 = total - p0                                        # a random split of each value over the two planes
        rows = {1: lambda: lib.mrcnn_conv3x3_winograd_heads_rows(batch, h, w, 1),
                2: lambda: lib.mrcnn_conv3x3_winograd_heads_rows(batch, h, w, 2),
                3: lambda: lib.mrcnn_conv3x3_winograd4_heads_rows(batch, h, w),
                4: lambda: batch * h * w}[mode]()
        idx = torch.from_numpy(_head_rows(mode, batch, h, w).reshape(-1))
        assert int(idx.max()) < rows and idx.unique().numel() == idx.numel()
        if mode == 3:
            part = torch.full((rows, 32), float("nan"))
            part[idx, :18] = p0.reshape(-1, 18)
            nhwc.append(p0 + bias)
        else:
            part = torch.full((2, rows, 32), float("nan"))
            part[0, idx, :18] = p0.reshape(-1, 18)
            part[1, idx, :18] = p1.reshape(-1, 18)
            nhwc.append((p0 + p1) + bias)
        parts.append(part)
    hs, ws, modes = ([v[i] for v in levels] for i in range(3))
    s1, d1 = _rpn([t.to(dev) for t in parts], hs, ws, modes, bias.to(dev), batch, dev)
    s0, d0 = _rpn([t.contiguous().to(dev) for t in nhwc], hs, ws, [0] * 5, None, batch, dev)
    assert not torch.isnan(s1).any() and not torch.isnan(d1).any()
    assert _bits_equal(d1, d0) and _bits_equal(s1, s0)
    assert _bits_equal(d0, torch.cat([t[..., 6:].reshape(batch, -1, 4) for t in nhwc], 1))


# ====================================================================================================== topk_desc
def _topk(s, k, dev):
    """s: device tensor [B, n] (any alignment). → top, order (host), ncand (host, int64 [B]).
    WHITE-BOX: ncand is read back from the caller-owned workspace, whose first `batch` uint32 are the candidate counts of
    the two-pass scheme (topk_layout in csrc/select.hip) — the only way to tell which of the kernel's regimes a case took."""
    from maskrcnn_amd._lib import lib
    b, n = s.shape
    top, order = _Out((b, k), F32, dev), _Out((b, k), I64, dev)
    nbytes = int(lib.mrcnn_topk_workspace_bytes(b))
    ws = _Out((nbytes,), torch.uint8, dev, fill=0xA5)
    _run(lib.mrcnn_topk_desc_f32, (s.data_ptr(), b, n, k, top.ptr, order.ptr, ws.ptr, nbytes), (top, order, ws))
    ncand = ws.t[:4 * b].cpu().numpy().view(np.uint32).astype(np.int64)
    return top.t.cpu(), order.t.cpu(), ncand


def _ref_topk(s, k):
    """descending, NaN first, ties by ascending index: ATen's stable sort on the CPU."""
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    return s.gather(1, order), order


def _assert_topk(s, k, top, order, tag):
    rt, ro = _ref_topk(s, k)
    nz = ~(rt == 0)                                            # the kernel orders -0.0 below +0.0, the CPU sort does not
    assert torch.equal(_bits(top)[nz], _bits(rt)[nz]) and bool((top[~nz] == 0).all()), tag
    assert torch.equal(order[nz], ro[nz]), tag
    for b in range(s.size(0)):
        assert order[b].unique().numel() == k and bool((s[b, order[b]] == 0)[~nz[b]].all()), tag


def _regime(row, k, ncand):
    """The branch of topk_finish_kernel a row takes (csrc/select.hip), from ncand and the data."""
    if ncand > 4096:
        return "exact"
    if k > 1024:
        return "lds"
    if ncand <= 1024:
        return "small"
    v = torch.sort(row, descending=True).values
    thr = v[k - 1]
    need, have = k - int((row > thr).sum()), int((row == thr).sum())
    return "trim-ties" if have != need else "trim"


def _run_topk_case(s, k, dev, tag, offset=False):
    if offset:   # base pointer one float past a 16-byte boundary: the scalar path of stream_row
        flat = torch.empty(s.numel() + 1, dtype=F32, device=dev)
        flat[1:] = s.reshape(-1).to(dev)
        sd = flat[1:].view(s.shape)
        assert sd.data_ptr() % 16 == 4
    else:
        sd = s.to(dev)
    top, order, ncand = _topk(sd, k, dev)
    _assert_topk(s, k, top, order, tag)
    return ncand


N_ANCHORS = 261888   # anchors of a 1024 x 1024 image


def test_topk_desc_reaches_each_of_its_five_regimes(dev):
    """One case per branch of topk_finish_kernel at n = 261888, the regime asserted through ncand (white-box, see _topk):
    ncand <= 1024; (1024, 4096] trimmed without ties at the cut; the same with more keys equal to the threshold than wanted;
    k > 1024 (sorted in LDS); ncand > 4096 (exact_topk_row). Plus the trained-like row: 1300 scores exactly 1.0 over a
    near-zero background, k = 1000 — the lowest indices must win."""
    g = torch.Generator().manual_seed(2100)
    uni = lambda: torch.rand(1, N_ANCHORS, generator=g)
    trained = torch.rand(1, N_ANCHORS, generator=g) * 1e-3
    trained[0, torch.randperm(N_ANCHORS, generator=g)[:1300]] = 1.0
    cases = [("uniform k500", uni(), 500, "small"),
             ("uniform k1000", uni(), 1000, "trim"),
             ("quantised k1000", torch.floor(uni() * 16384) / 16384, 1000, "trim-ties"),
             ("uniform k2000", uni(), 2000, "lds"),
             ("uniform k4096", uni(), 4096, "exact"),
             ("trained-like k1000", trained, 1000, "trim-ties")]
    seen = set()
    for tag, s, k, want in cases:
        ncand = _run_topk_case(s, k, dev, tag)
        got = _regime(s[0], k, int(ncand[0]))
        print(f"topk regime: {tag}: ncand {int(ncand[0])} -> {got}")
        assert k <= ncand[0] and got == want, (tag, int(ncand[0]), got)
        seen.add(got)
    assert seen == {"small", "trim", "trim-ties", "lds", "exact"}
    top, order, _ = _topk(trained.to(dev), 1000, dev)
    assert bool((top == 1.0).all()) and torch.equal(order[0], (trained[0] == 1.0).nonzero().flatten()[:1000])


def test_topk_desc_sorted_equal_full_and_misaligned_rows(dev):
    """Sorted rows (they defeat the per-thread-maxima bound: ascending with k = 2000 must take exact_topk_row), all-equal rows,
    k == n for n in {1, 4095, 4096}, and batch 5 with n % 4 != 0 on an aligned and on a one-float-offset base pointer (rows
    of every alignment, the scalar tail of stream_row)."""
    g = torch.Generator().manual_seed(2200)
    asc = torch.sort(torch.rand(1, N_ANCHORS, generator=g), dim=1).values
    for k in (1000, 2000):
        ncand = _run_topk_case(asc, k, dev, ("ascending", k))
        print(f"topk ascending row k {k}: ncand {int(ncand[0])}")
        if k == 2000:
            assert ncand[0] > 4096
        _run_topk_case(asc.flip(1).contiguous(), k, dev, ("descending", k))
    # 5000 equal scores are more candidates than the LDS sort holds: exact_topk_row sorts exactly k composites, k = 1 among them
    # (no sort step at all) and k = 65 (one past a wave)
    for n, k in ((3000, 1000), (N_ANCHORS, 1000), (N_ANCHORS, 4096), (5000, 5), (5000, 1), (5000, 65)):
        s = torch.full((2, n), 0.25)
        top, order, ncand = _topk(s.to(dev), k, dev)
        assert torch.equal(order, torch.arange(k).expand(2, k)) and bool((top == 0.25).all()), (n, k)
    for n in (1, 4095, 4096):
        _run_topk_case(torch.randn(3, n, generator=g), n, dev, ("k == n", n))
    for n, k in ((4099, 77), (70001, 1000), (12347, 4096), (9, 9), (6, 1)):
        s = torch.randn(5, n, generator=g)
        for offset in (False, True):
            _run_topk_case(s, k, dev, ("batch 5", n, k, offset), offset=offset)


def test_topk_desc_non_finite_and_signed_zero_scores(dev):
    """NaN of both signs (0x7FC00000 and the 0xFFC00000 that inf - inf gives on x86), +-inf and +-0 mixed into the rows, against
    torch.sort(stable=True, descending=True) on the CPU: every NaN first, in index order."""
    g = torch.Generator().manual_seed(2300)
    s = torch.randn(4, 50000, generator=g)
    s[1] = torch.randint(0, 4, (50000,), generator=g).float() / 3.0 - 0.5
    for b, (npos, nneg) in enumerate(((300, 300), (3, 5), (0, 700), (2500, 2500))):
        p = torch.randperm(50000, generator=g)
        s[b, p[:npos]] = float("nan")
        s[b, p[npos:npos + nneg]] = _neg_nan()
        s[b, p[6000:6400]] = float("inf")
        s[b, p[7000:7400]] = float("-inf")
        s[b, p[8000:8400]] = -0.0
        s[b, p[9000:9400]] = 0.0
    assert int((_bits(s) == -4194304).sum()) == 300 + 5 + 700 + 2500      # 0xFFC00000 survived the host ops
    for k in (1, 64, 600, 1000, 4096):
        _run_topk_case(s, k, dev, ("specials", k))
        _run_topk_case(s[:, :49999].contiguous(), k, dev, ("specials, odd n", k), offset=True)
    # a row of nothing but NaNs of both signs: index order
    s = torch.full((1, 5000), float("nan"))
    s[0, ::2] = _neg_nan()
    top, order, _ = _topk(s.to(dev), 1000, dev)
    assert torch.equal(order[0], torch.arange(1000)) and _bits_equal(top, s[:, :1000])


@pytest.mark.timeout(1500)
def test_topk_desc_row_longer_than_2_to_31(dev):
    """n = 2^31 + 4099 (an 8 GiB row), batch 1, k = 1000: background rand * 0.5 generated on the device, 1000 distinct winners
    in (0.5, 1] planted at chosen indices, among them 0, 2^31 - 1, 2^31 and n - 1 — the expected answer is known by
    construction. Exercises the 64-bit element offsets and the 32-bit complemented index of the candidate keys."""
    n, k = (1 << 31) + 4099, 1000
    torch.cuda.empty_cache()
    g = torch.Generator(device=dev).manual_seed(2400)
    s = torch.empty(n, dtype=F32, device=dev)
    step = 1 << 28
    for a in range(0, n, step):
        s[a:a + step].uniform_(0.0, 0.5, generator=g)
    assert float(s[a:].max()) < 0.5
    hg = torch.Generator().manual_seed(2401)
    idx = torch.randint(0, n, (k - 8,), generator=hg, dtype=I64)
    idx = torch.cat([idx, torch.tensor([0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) // 2 + 4096, n - 2, n - 1])])
    assert idx.unique().numel() == k
    val = 0.5 + (torch.randperm(k, generator=hg).float() + 1) / 2000.0          # distinct, in (0.5, 1]
    assert val.unique().numel() == k and float(val.min()) > 0.5 and float(val.max()) <= 1.0
    for a in range(0, n, step):
        m = (idx >= a) & (idx < a + step)
        s[a:a + step][(idx[m] - a).to(dev)] = val[m].to(dev)
    top, order, ncand = _topk(s.view(1, n), k, dev)
    del s
    torch.cuda.empty_cache()
    print(f"topk n = 2^31 + 4099: ncand {int(ncand[0])}")
    by = torch.sort(val, descending=True)
    assert torch.equal(top[0], by.values) and torch.equal(order[0], idx[by.indices])


# ================================================================================================ proposal_decode
def _proposal_decode(anchors, deltas, order, top, h, w, dev):
    from maskrcnn_amd._lib import c_f32, lib
    b, k = order.shape
    dets = _Out((b, k, 5), F32, dev)
    a, d, o, t = anchors.to(dev), deltas.to(dev), order.to(dev), top.to(dev)
    _run(lib.mrcnn_proposal_decode_f32, (a.data_ptr(), d.data_ptr(), o.data_ptr(), t.data_ptr(), b, a.size(0), k,
                                         _arr(c_f32, STD), float(h), float(w), dets.ptr), (dets,))
    return dets.t.cpu()


def _refine64(boxes, d):
    """boxes_refine (data.py:124-148) in float64; d already multiplied by the std dev."""
    h, w = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cy, cx = boxes[:, 0] + 0.5 * h + d[:, 0] * h, boxes[:, 1] + 0.5 * w + d[:, 1] * w
    with np.errstate(over="ignore"):
        h, w = h * np.exp(d[:, 2]), w * np.exp(d[:, 3])
    y1, x1 = cy - 0.5 * h, cx - 0.5 * w
    return np.stack([y1, x1, y1 + h, x1 + w], 1)


def test_proposal_decode_exact_random_and_overflowing(dev):
    """(a) zero deltas on anchors whose coordinates are multiples of 1/4 (every fp32 op exact, expf(0) == 1): the clamped anchor
    bit for bit, for anchors inside, partly and wholly outside the image, `order` holding the first and the last anchor and
    repeats, B*k = 231 (not a multiple of 256). (b) random deltas against float64, rtol 1e-6 / atol 1e-4 as
    test_rpn_scores_deltas_and_proposal_decode. (c) dh*std, dw*std of +-100: expf overflows to inf, y1 = -inf and
    y2 = -inf + inf = NaN. The pinned contract (maskrcnn_hip.h): fminf(fmaxf(v, lo), hi) turns the NaN into the lower bound —
    every coordinate finite and inside [0,H] x [0,W], the overflowing side exactly (0, 0); underflow gives width 0."""
    g = torch.Generator().manual_seed(3100)
    b, k, a, ih, iw = 3, 77, 5000, 1024, 768
    anchors = torch.randint(-1600, 5600, (a, 4), generator=g).float() / 4
    anchors[0] = torch.tensor([-50.0, -60.0, -10.0, -1.0])                     # wholly outside
    anchors[a - 1] = torch.tensor([1000.0, 700.0, 1100.25, 800.5])             # partly outside
    order = torch.randint(0, a, (b, k), generator=g)
    order[:, 0], order[:, 1], order[:, 2], order[:, 3] = 0, a - 1, a - 1, 0
    top = torch.rand(b, k, generator=g)
    top[0, 5], top[1, 6] = float("nan"), _neg_nan()                            # the score column is a copy
    hi = torch.tensor([ih, iw, ih, iw], dtype=F32)
    dets = _proposal_decode(anchors, torch.zeros(b, a, 4), order, top, ih, iw, dev)
    assert _bits_equal(dets[..., :4], torch.minimum(torch.clamp_min(anchors[order], 0.0), hi))
    assert _bits_equal(dets[..., 4], top)
    # (b)
    anchors = torch.rand(a, 4, generator=g) * 900 - 50
    anchors[:, 2:] = anchors[:, :2] + torch.rand(a, 2, generator=g) * 300 + 1
    deltas = torch.randn(b, a, 4, generator=g)
    dets = _proposal_decode(anchors, deltas, order, top, ih, iw, dev)
    std, hi64 = np.array(STD), hi.double().numpy()
    for i in range(b):
        want = np.clip(_refine64(anchors[order[i]].double().numpy(), deltas[i][order[i]].double().numpy() * std), 0.0, hi64)
        np.testing.assert_allclose(dets[i, :, :4].double().numpy(), want, rtol=1e-6, atol=1e-4)
    # (c)
    big = deltas.clone()
    rows = order[0, :40]
    big[0, rows[0:10], 2] = 500.0      # dh * std = +100
    big[0, rows[10:20], 3] = 500.0
    big[0, rows[20:30], 2] = -500.0    # dh * std = -100
    big[0, rows[30:40], 3] = -500.0
    big[0, rows[0:5], 0] = 1e38        # and a centre that overflows
    dets = _proposal_decode(anchors, big, order, top, ih, iw, dev)
    box = dets[..., :4]
    assert bool(torch.isfinite(box).all()) and bool((box >= 0).all()) and bool((box <= hi).all())
    first = {int(r): j for j, r in reversed(list(enumerate(order[0].tolist())))}   # repeated indices: any slot of the anchor
    for j, r in enumerate(rows.tolist()):
        y1, x1, y2, x2 = dets[0, first[r], :4].tolist()
        if big[0, r, 2] == 500.0:
            assert (y1, y2) == (0.0, 0.0), (j, y1, y2)                             # -inf -> 0 and NaN -> 0
        if big[0, r, 3] == 500.0:
            assert (x1, x2) == (0.0, 0.0), (j, x1, x2)
        if big[0, r, 2] == -500.0:
            assert y1 == y2
        if big[0, r, 3] == -500.0:
            assert x1 == x2
    same = torch.ones(b, k, dtype=torch.bool)
    same[0] = ~torch.isin(order[0], rows)
    clean = _proposal_decode(anchors, deltas, order, top, ih, iw, dev)
    assert torch.equal(_bits(dets)[same], _bits(clean)[same])                      # no other row moved


# =============================================================================================== detection_decode
def _detection_decode(lg, lg_stride, bb, bb_stride, rois, counts, windows, b, p, c, ih, iw, min_conf, dev):
    """lg / bb: device pointers (int) of row 0 with their row strides in elements."""
    from maskrcnn_amd._lib import c_f32, lib
    dets, nms, cls = _Out((b, p, 5), F32, dev), _Out((b, p), I32, dev), _Out((b, p), I64, dev)
    r, n, w = rois.to(dev).contiguous(), counts.to(dev), windows.to(dev).contiguous()
    _run(lib.mrcnn_detection_decode_f32, (lg, lg_stride, bb, bb_stride, r.data_ptr(), n.data_ptr(), w.data_ptr(), b, p, c,
                                          _arr(c_f32, STD), float(ih), float(iw), float(min_conf), dets.ptr, nms.ptr,
                                          cls.ptr), (dets, nms, cls))
    return dets.t.cpu(), nms.t.cpu(), cls.t.cpu()


def _decode(logits, bbox, rois, counts, windows, ih, iw, min_conf, dev, strided=False):
    """logits [B*P, C], bbox [B*P, C, 4], rois [B, P, 4] on the host. strided: rows inside wider buffers whose other columns
    hold NaN."""
    (b, p, _), c = rois.shape, logits.size(1)
    if strided:
        lw = torch.full((b * p, c + 5), float("nan"))
        lw[:, 2:2 + c] = logits
        bw = torch.full((b * p, 4 * c + 8), float("nan"))
        bw[:, 4:4 + 4 * c] = bbox.reshape(b * p, 4 * c)
        lw, bw = lw.to(dev), bw.to(dev)
        return _detection_decode(lw.data_ptr() + 8, c + 5, bw.data_ptr() + 16, 4 * c + 8, rois, counts, windows, b, p, c, ih,
                                 iw, min_conf, dev)
    lg, bb = logits.contiguous().to(dev), bbox.contiguous().to(dev)
    return _detection_decode(lg.data_ptr(), c, bb.data_ptr(), 4 * c, rois, counts, windows, b, p, c, ih, iw, min_conf, dev)


def _decode_ref(logits, bbox, rois, counts, windows, ih, iw):
    """float64 restatement of mrcnn_detection_decode_f32's contract (maskrcnn_hip.h). → dict of numpy arrays over the B*P slots:
    empty (no record: slot past the count, or a live row whose softmax is NaN), ids, score, pre (clipped box before rounding)."""
    (b, p, _), c = rois.shape, logits.size(1)
    lg = logits.double().numpy()
    slot, img = np.arange(b * p) % p, np.arange(b * p) // p
    live = slot < counts.numpy()[img]
    nan_row = np.isnan(lg).any(1) | np.isposinf(lg).any(1) | np.isneginf(lg).all(1)
    ok = live & ~nan_row
    safe = np.where(ok[:, None], lg, 0.0)
    ids = np.argmax(safe, 1)                                    # the first index of the maximum
    with np.errstate(under="ignore"):
        score = 1.0 / np.exp(safe - safe.max(1, keepdims=True)).sum(1)
    d = bbox.double().numpy()[np.arange(b * p), ids] * np.array(STD)
    d = np.where(ok[:, None], d, 0.0)
    box = _refine64(rois.reshape(-1, 4).double().numpy(), d) * np.array([ih, iw, ih, iw], dtype=np.float64)
    w = windows.double().numpy()[img]
    pre = np.stack([np.clip(box[:, 0], w[:, 0], w[:, 2]), np.clip(box[:, 1], w[:, 1], w[:, 3]),
                    np.clip(box[:, 2], w[:, 0], w[:, 2]), np.clip(box[:, 3], w[:, 1], w[:, 3])], 1)
    return dict(empty=~ok, ids=ids, score=score, pre=pre, slot=slot)


def _assert_decode(got, ref, min_conf, tag, exact_boxes=False):
    """→ (coordinates skipped, coordinates compared)."""
    dets, nms, cls = (t.reshape(-1, *t.shape[2:]).numpy() for t in got)
    e, ok = ref["empty"], ~ref["empty"]
    assert not dets[e].any() and not cls[e].any() and np.array_equal(nms[e], -(ref["slot"][e] + 1)), tag   # the empty record
    assert np.array_equal(cls[ok], ref["ids"][ok]), tag
    assert np.abs(dets[ok, 4].astype(np.float64) - ref["score"][ok]).max(initial=0.0) <= 1e-6, tag
    valid = ok & (ref["ids"] > 0)
    if min_conf > 0:
        valid &= dets[:, 4] >= np.float32(min_conf)
    assert np.array_equal(nms > 0, valid) and np.array_equal(nms[valid], ref["ids"][valid]), tag
    for row, v in zip(nms.reshape(got[1].shape), valid.reshape(got[1].shape)):        # excluded slots: unique negatives
        assert (row[~v] < 0).all() and np.unique(row[~v]).size == int((~v).sum()), tag
    pre = ref["pre"][ok]
    near_half = np.zeros_like(pre, dtype=bool) if exact_boxes else np.abs(pre - np.floor(pre) - 0.5) < 1e-3
    assert np.array_equal(dets[ok, :4][~near_half], np.rint(pre)[~near_half].astype(np.float32)), tag
    return int(near_half.sum()), int(near_half.size)


def _decode_inputs(g, b, p, c, ih=512, iw=640):
    logits = torch.randn(b * p, c, generator=g) * 2
    bbox = torch.randn(b * p, c, 4, generator=g) * 0.3
    ctr = torch.rand(b, p, 2, generator=g)
    hw = torch.rand(b, p, 2, generator=g) * 0.3 + 0.02
    rois = torch.cat([ctr - hw / 2, ctr + hw / 2], -1).clamp(0, 1)
    return logits, bbox, rois


def test_detection_decode_class_counts_roi_counts_strides_against_float64(dev):
    """C in {1, 2, 3, 63, 64, 65, 81, 128, 129} (one lane, one pass, one pass + 1, two passes + 1) x B*P in {1, 3, 37, 1000}
    (the grid is (B*P + 3) / 4 wavefront quads), contiguous and as row-strided views into wider NaN-filled buffers, roi_counts of
    0 and P among them, windows strictly inside the image and degenerate (a line), logits at +-1e4, min_confidence 0 and 0.3.
    Against float64: arg-max exact (first index), scores within 1e-6 (test_detection_decode_vs_oracle_math's bound), boxes
    equal after rounding except coordinates whose float64 value lies within 1e-3 of a .5, which are skipped: at most 1 % of
    them may be (uniform inputs: 2e-3 expected; the float64 reference alone decides which: 94 of 46512 here, 2.0e-3)."""
    g = torch.Generator().manual_seed(4100)
    ih, iw = 512, 640
    skipped = total = 0
    for c in (1, 2, 3, 63, 64, 65, 81, 128, 129):
        for b, p, counts in ((1, 1, [1]), (3, 1, [1, 0, 1]), (1, 37, [20]), (2, 500, [500, 123])):
            logits, bbox, rois = _decode_inputs(g, b, p, c, ih, iw)
            for r in range(0, b * p, 5):                        # saturated rows: one logit at 1e4, the others at -1e4
                logits[r] = -1e4
                logits[r, int(torch.randint(0, c, (1,), generator=g))] = 1e4
            windows = torch.tensor([[0., 0., ih, iw], [64., 32., 448., 600.], [100., 50., 100., 300.]])[:b].contiguous()
            if b == 1:
                windows = torch.tensor([[64., 32., 448., 600.]]) if p == 37 else windows
            counts = torch.tensor(counts, dtype=I32)
            ref = _decode_ref(logits, bbox, rois, counts, windows, ih, iw)
            for min_conf in (0.0, 0.3):
                strided = (c + p) % 2 == 0 or min_conf > 0
                got = _decode(logits, bbox, rois, counts, windows, ih, iw, min_conf, dev, strided=strided)
                s, t = _assert_decode(got, ref, min_conf, (c, b, p, min_conf, strided))
                skipped, total = skipped + s, total + t
    print(f"detection_decode: {skipped} of {total} coordinates within 1e-3 of a .5 skipped ({skipped / total:.2e})")
    assert skipped <= 0.01 * total


def test_detection_decode_ties_rounding_and_threshold_exactly(dev):
    """Exact cases. Arg-max ties: the first index wins (numpy.argmax). Rounding: zero deltas, a 512 x 512 image and RoIs at pixel
    coordinates k + 0.5 (every fp32 op exact) — half to even, for even and odd k. min_confidence equal to a representable
    score: two equal logits and the rest -inf give exactly 0.5, which `>=` keeps and the next float up drops."""
    g = torch.Generator().manual_seed(4200)
    b, p, c, ih, iw = 1, 64, 81, 512, 512
    logits = torch.randint(-3, 4, (b * p, c), generator=g).float()          # heavy ties
    logits[0] = 0.0                                                          # all equal: class 0
    logits[1, 1:] = 2.0                                                      # class 1 first among 80 equals
    logits[2], logits[2, 80] = -1.0, 5.0
    bbox = torch.zeros(b * p, c, 4)
    k = torch.arange(p).float() * 3 + 10                                     # even and odd k
    rois = torch.stack([(k + 0.5) / 512, (k + 1.5) / 512, (k + 40.5) / 512, (k + 101.5) / 512], 1).view(1, p, 4)
    counts, windows = torch.tensor([p], dtype=I32), torch.tensor([[0., 0., 512., 512.]])
    dets, nms, cls = _decode(logits, bbox, rois, counts, windows, ih, iw, 0.0, dev)
    assert np.array_equal(cls[0].numpy(), np.argmax(logits.numpy(), 1))
    even = lambda v: torch.where(v % 2 == 0, v, v + 1)                       # k + 0.5 -> the even neighbour
    want = torch.stack([even(k), even(k + 1), even(k + 40), even(k + 101)], 1)
    assert torch.equal(dets[0, :, :4], want) and {0.0, 1.0} == set((want[:, 0] - k).tolist())
    _assert_decode((dets, nms, cls), _decode_ref(logits, bbox, rois, counts, windows, ih, iw), 0.0, "ties", exact_boxes=True)
    # the threshold
    logits = torch.full((b * p, c), float("-inf"))
    logits[:, 3] = logits[:, 7] = 1.25
    logits[1, 0], logits[1, 7] = 1.25, float("-inf")                         # background ties first: invalid whatever the score
    up = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    for min_conf, keeps in ((0.5, True), (up, False)):
        dets, nms, cls = _decode(logits, bbox, rois, counts, windows, ih, iw, min_conf, dev)
        assert bool((dets[0, :, 4] == 0.5).all())
        assert bool((cls[0, 2:] == 3).all()) and int(cls[0, 1]) == 0
        assert bool((nms[0, 2:] == 3).all()) == keeps and bool((nms[0, 2:] < 0).all()) == (not keeps)
        assert int(nms[0, 1]) == -2


NONFINITE_KINDS = ("one NaN", "one +inf", "all NaN", "all -inf", "some -inf")


def _poison(row, kind, g):
    c = row.numel()
    j = int(torch.randint(0, c, (1,), generator=g))
    if kind == "one NaN":
        row[j] = float("nan") if j % 2 else _neg_nan()
    elif kind == "one +inf":
        row[j] = float("inf")
    elif kind == "all NaN":
        row[:] = float("nan")
    elif kind == "all -inf":
        row[:] = float("-inf")
    else:
        row[torch.randperm(c, generator=g)[:c // 2]] = float("-inf")
        row[j] = 3.0                                                         # a finite maximum survives


@pytest.mark.parametrize("c", [81, 129])
@pytest.mark.parametrize("group", ["partial", "no_maximum"])
def test_detection_decode_rows_whose_softmax_is_nan_are_empty_slots(dev, c, group):
    """A live row with a NaN logit, a +inf logit, nothing but NaN, or nothing but -inf has a NaN softmax in the reference
    (F.softmax, then torch.max -> index 0 -> background, dropped): the empty-slot record, with nothing read from its bbox row
    (NaN there too), at slot 0 of image 0, at wave and block boundaries and at the last slot. A row with some -inf and a
    finite maximum decodes normally. Every other row is bit-identical to a run where those rows hold benign values.
    (Before the fix the first two became valid detections with a NaN score — the top detection after NMS's NaN-first order —
    and the rows without a maximum indexed bbox with 0x7fffffff * 4: the "no_maximum" group must never run on a kernel
    without the fix, tests/test_boundary.py restates that loop on the host instead.)"""
    names = {"partial": ("one NaN", "one +inf", "some -inf"), "no_maximum": ("all NaN", "all -inf", "some -inf")}[group]
    g = torch.Generator().manual_seed(4300 + c)
    b, p, ih, iw = 2, 41, 512, 640
    logits, bbox, rois = _decode_inputs(g, b, p, c, ih, iw)
    logits[:, 0] -= 2.0                                                      # mostly foreground
    counts, windows = torch.tensor([p, 30], dtype=I32), torch.tensor([[0., 0., ih, iw], [64., 0., 448., 640.]])
    rows = [0, 1, 2, 3, 4, 7, 17, 22, 36, 40, p + 0, p + 5, p + 11, p + 28, p + 29]       # live rows of both images
    kinds = {r: names[i % 3] for i, r in enumerate(rows)}
    bad_l, bad_b = logits.clone(), bbox.clone()
    for r, kind in kinds.items():
        _poison(bad_l[r], kind, g)
        if kind != "some -inf":
            bad_b[r] = float("nan")
    ref = _decode_ref(bad_l, bad_b, rois, counts, windows, ih, iw)
    assert [bool(ref["empty"][r]) for r in rows] == [kinds[r] != "some -inf" for r in rows]
    untouched = torch.ones(b * p, dtype=torch.bool)
    untouched[rows] = False
    for min_conf in (0.0, 0.3):
        for strided in (False, True):
            clean = _decode(logits, bbox, rois, counts, windows, ih, iw, min_conf, dev, strided=strided)
            got = _decode(bad_l, bad_b, rois, counts, windows, ih, iw, min_conf, dev, strided=strided)
            for t in got:
                assert not torch.isnan(t.float()).any()
            assert int(got[2].max()) < c and int(got[2].min()) >= 0
            _assert_decode(got, ref, min_conf, (c, min_conf, strided))
            for a_, b_ in zip(got, clean):
                assert torch.equal(_bits(a_.reshape(b * p, -1))[untouched], _bits(b_.reshape(b * p, -1))[untouched])
            for r, kind in kinds.items():
                if kind != "some -inf":
                    assert int(got[1].view(-1)[r]) == -(r % p + 1) and not got[0].view(-1, 5)[r].any(), (r, kind)


# =========================================================================== proposal_select / detection_select
SELECT_SIZES = (1, 2, 1023, 1024, 1025, 4095, 4096)


def _keep_rows(g, b, n, counts):
    keep = torch.full((b, n), -1, dtype=I64)
    for i, cnt in enumerate(counts):
        keep[i, :cnt] = torch.sort(torch.randperm(n, generator=g)[:cnt]).values
    return keep


@pytest.mark.parametrize("p", SELECT_SIZES)
def test_proposal_select_sizes_and_counts(dev, p):
    """proposal_count P in {1, 2, 1023, 1024, 1025, 4095, 4096} with k == P and k > P, keep_counts of 0, 1, P and k; entries of
    `keep` past the count are -1 and must not be read. Bit for bit against the gather + divide of model.py:1366-1374."""
    from maskrcnn_amd._lib import lib
    g = torch.Generator().manual_seed(5100 + p)
    norm = torch.tensor([1024.0, 768.0, 1024.0, 768.0])
    for k in sorted({p, min(p + 37, 4096)}):
        counts = [0, 1, min(p, k), k, int(torch.randint(0, k + 1, (1,), generator=g))]
        b = len(counts)
        dets = torch.rand(b, k, 5, generator=g) * 1000
        keep = _keep_rows(g, b, k, counts)
        rois, cnt = _Out((b, p, 4), F32, dev), _Out((b,), I32, dev)
        d, kp, kc = dets.to(dev), keep.to(dev), torch.tensor(counts, dtype=I32, device=dev)
        _run(lib.mrcnn_proposal_select_f32, (d.data_ptr(), kp.data_ptr(), kc.data_ptr(), b, k, p, 1024.0, 768.0, rois.ptr,
                                             cnt.ptr), (rois, cnt))
        assert cnt.t.cpu().tolist() == [min(v, p) for v in counts]
        for i, v in enumerate(counts):
            n = min(v, p)
            want = torch.zeros(p, 4)
            want[:n] = dets[i, keep[i, :n], :4] / norm
            assert _bits_equal(rois.t[i], want), (p, k, i)


def _detection_select(dets, nms_cls, class_ids, keep, counts, d, dev):
    from maskrcnn_amd._lib import lib
    b, p, _ = dets.shape
    outs = [_Out((b, d), I64, dev), _Out((b, d), F32, dev), _Out((b, d, 4), F32, dev), _Out((b, d, 4), F32, dev),
            _Out((b,), I32, dev)]
    ins = [t.to(dev) for t in (dets, nms_cls, class_ids, keep, counts)]
    _run(lib.mrcnn_detection_select_f32, (*[t.data_ptr() for t in ins], b, p, d, 1024.0, 512.0, *[o.ptr for o in outs]), outs)
    return [o.t.cpu() for o in outs]


def _detection_select_ref(dets, nms_cls, class_ids, keep, count, d):
    p = dets.size(0)
    kept = torch.zeros(p, dtype=torch.bool)
    kept[keep[:count]] = True
    cand = (kept & (nms_cls > 0)).nonzero().flatten()
    return cand[torch.sort(dets[cand, 4], descending=True, stable=True).indices][:d]      # NaN first, ties by index


@pytest.mark.parametrize("p", SELECT_SIZES)
def test_detection_select_sizes_counts_nan_and_ties(dev, p):
    """rois_per_image P in {1, 2, 1023, 1024, 1025, 4095, 4096} (the register sort and the LDS sort meet at 1024); max_instances
    of 1, of P (more than there are candidates) and in between; keep_counts of 0 and P; an all-background image; scores
    quantised to eight values so that equal scores straddle the cut; NaN scores of both signs, which rank first in index order
    (torch.sort(stable=True, descending=True)). Images 5 and 6: exactly one candidate and exactly min(65, P) candidates, all
    foreground (the LDS sort of P > 1024 with a single real key, and with one more than a wave of them). Bit for bit."""
    g = torch.Generator().manual_seed(5200 + p)
    b = 7
    dets = torch.rand(b, p, 5, generator=g)
    dets[..., :4] = (dets[..., :4] * 900).round()
    dets[0, :, 4] = torch.randint(0, 8, (p,), generator=g).float() / 8            # ties across every cut
    dets[3, :, 4] = torch.randint(0, 3, (p,), generator=g).float() - 1.0          # -1, 0, 1
    for i in (0, 3, 4):
        q = torch.randperm(p, generator=g)
        dets[i, q[:max(1, p // 50)], 4] = float("nan")
        dets[i, q[p // 50 + 1:p // 25 + 2], 4] = _neg_nan()
    class_ids = torch.randint(0, 81, (b, p), generator=g)
    class_ids[2] = 0                                                               # all background
    class_ids[0] = class_ids[0].clamp_min(1)                                       # all foreground
    class_ids[5:] = class_ids[5:].clamp_min(1)
    nms_cls = torch.where(class_ids > 0, class_ids, -torch.arange(1, p + 1).expand(b, p)).to(I32)
    counts = [p, 0, p, p, int(torch.randint(0, p + 1, (1,), generator=g)), 1, min(65, p)]
    keep = _keep_rows(g, b, p, counts)
    for d in sorted({1, p, min(p, 100), max(1, p // 2)}):
        ids, scores, boxes, rois, cnt = _detection_select(dets, nms_cls, class_ids, keep, torch.tensor(counts, dtype=I32), d, dev)
        norm = torch.tensor([1024.0, 512.0, 1024.0, 512.0])
        for i in range(b):
            order = _detection_select_ref(dets[i], nms_cls[i], class_ids[i], keep[i], counts[i], d)
            n = order.numel()
            assert int(cnt[i]) == n, (p, d, i)
            assert torch.equal(ids[i, :n], class_ids[i, order]) and not ids[i, n:].any(), (p, d, i)
            assert _bits_equal(scores[i, :n], dets[i, order, 4]) and _bits_equal(scores[i, n:], torch.zeros(d - n)), (p, d, i)
            assert _bits_equal(boxes[i, :n], dets[i, order, :4]) and not boxes[i, n:].any(), (p, d, i)
            assert _bits_equal(rois[i, :n], dets[i, order, :4] / norm) and not rois[i, n:].any(), (p, d, i)
        assert int(cnt[1]) == 0 and int(cnt[2]) == 0


# ==================================================================================================== stage level
def _stage_cfgs(oracle, d):
    from maskrcnn_amd.config import InferenceConfig
    cfg = InferenceConfig(image_height=1024, image_width=1024, pre_nms_limit=1000, proposal_count=1000,
                          detection_max_instances=d)
    ocfg = oracle.Cfg(1024, 1024, PRE_NMS_LIMIT=1000, RPN_NMS_MAX_ROIS_NUM=1000, DETECTION_MAX_INSTANCES=d)
    return cfg, ocfg


def _trained_like_rpn(g, anchors):
    """Scores and deltas of three images over the 261888 anchors of a 1024^2 image: image 0 with 3000 scores exactly 1.0 in 30
    runs of neighbouring anchors (three times the top-k: ties across the cut), image 1 with about 600 of them plus graded runs,
    image 2 with no foreground at all."""
    a = anchors.size(0)
    scores = torch.rand(3, a, generator=g) * 1e-3
    for img, (runs, length) in enumerate(((30, 100), (7, 100))):
        starts = torch.randint(0, 190000, (runs,), generator=g)                   # clustered: P2 anchors, neighbours in x
        for s0 in starts.tolist():
            scores[img, s0:s0 + length] = 1.0
    for s0 in torch.randint(0, a - 200, (10,), generator=g).tolist():
        scores[1, s0:s0 + 150] = torch.rand(150, generator=g) * 0.5 + 0.45
    deltas = torch.randn(3, a, 4, generator=g) * 0.5
    return scores, deltas


def _rows_match_as_sets(got, want, atol):
    d = (got[:, None, :] - want[None, :, :]).abs().amax(dim=2)
    return got.size(0) == want.size(0) and (got.size(0) == 0 or
                                            (d.min(dim=1).values.max().item() <= atol and d.min(dim=0).values.max().item() <= atol))


@pytest.fixture(scope="module")
def stage(dev, oracle):
    from maskrcnn_amd.anchors import pyramid_anchors
    from maskrcnn_amd.pipeline import MaskRCNNInference
    cfg, ocfg = _stage_cfgs(oracle, 1000)
    anchors = pyramid_anchors(cfg)
    assert anchors.size(0) == N_ANCHORS and torch.equal(anchors.cpu(), oracle.anchors_for(ocfg))
    g = torch.Generator().manual_seed(6100)
    scores, deltas = _trained_like_rpn(g, anchors)
    ns = SimpleNamespace(cfg=cfg, anchors=anchors.to(dev).contiguous())
    rois, counts, dets = MaskRCNNInference.proposals(ns, scores.to(dev), deltas.to(dev))
    torch.cuda.synchronize()
    return dict(cfg=cfg, ocfg=ocfg, anchors=anchors.cpu(), scores=scores, deltas=deltas, rois=rois.cpu(), counts=counts.cpu(),
                dets=dets.cpu(), g=g)


def test_proposals_stage_on_trained_like_scores(stage, oracle):
    """MaskRCNNInference.proposals (through a SimpleNamespace, as refine.py calls it) on 3 x 261888 trained-like scores, against
    oracle.rpn_refine per image as test_proposals_stage does: the score column equal; the dets equal (1e-3: expf ulps) to the
    decode of the anchors a STABLE descending sort picks — the kernel's documented tie rule, which decides who survives the
    cut among image 0's 3000 scores of exactly 1.0 —, and as a set equal to the reference's own dets wherever the score is
    above the cut's (ATen's unstable sort may order and cut ties differently); NMS bit-exact on the dets the HIP path used."""
    s, ocfg = stage, stage["ocfg"]
    for b in range(3):
        sc = s["scores"][b]
        rpn_class = torch.stack([1 - sc, sc], 1).unsqueeze(0)
        _, want = oracle.rpn_refine(rpn_class, s["deltas"][b].unsqueeze(0), s["anchors"], ocfg, return_dets=True)
        got = s["dets"][b]
        assert torch.equal(got[:, 4], want[:, 4]), b
        order = torch.sort(sc, descending=True, stable=True).indices[:1000]
        mine = oracle.boxes_clamp(oracle.boxes_refine(s["anchors"][order], oracle.boxes_scale(s["deltas"][b][order], STD)),
                                  [0, 0, 1024, 1024])
        assert torch.allclose(got[:, :4], mine, rtol=0, atol=1e-3), b
        above = got[:, 4] > got[-1, 4]
        if b == 0:
            assert int(above.sum()) == 0 and int((sc == 1.0).sum()) >= 2900      # the whole top-k is one tie group
        assert _rows_match_as_sets(got[above, :4], want[want[:, 4] > want[-1, 4], :4], 1e-3), b
        keep = oracle.nms(got, ocfg.RPN_NMS_THRESHOLD)[:ocfg.RPN_NMS_MAX_ROIS_NUM]
        n = int(s["counts"][b])
        assert n == keep.numel() and n >= 1
        assert torch.equal(s["rois"][b, :n], got[keep, :4] / 1024.0) and not s["rois"][b, n:].any(), b


def test_detections_stage_with_saturated_and_poisoned_rows(stage, oracle, dev):
    """MaskRCNNInference.detections on the proposals above: class logits with saturated winners (score exactly 1.0 in thousands
    of rows), rows poisoned with NaN / +inf / all NaN / all -inf, and image 2 all background. Against oracle.mrn_refine per
    image, given softmax(logits) as the reference's classifier would produce it (NaN rows: torch.max picks class 0, so both
    sides drop them): with detection_max_instances = 1000 nothing is cut, so the detections compare as sets whatever the
    reference's unstable sort does with ties — class ids and boxes exact, scores within 1e-6. Then exactly and in order
    against the class-aware NMS (oracle.nms) and a stable sort run on the dets the HIP decode produced; and
    detection_max_instances = 50 returns the first 50 of the same order."""
    from maskrcnn_amd import ops
    from maskrcnn_amd.pipeline import MaskRCNNInference
    s, ocfg, g = stage, stage["ocfg"], torch.Generator().manual_seed(6200)
    b, p, c = 3, 1000, 81
    logits = torch.randn(b * p, c, generator=g)
    winners = torch.randint(0, c, (b * p,), generator=g)
    winners[torch.rand(b * p, generator=g) < 0.3] = 0
    sat = torch.rand(b * p, generator=g) < 0.6
    logits[sat, winners[sat]] = 30.0
    logits[2 * p:] = torch.randn(p, c, generator=g) * 0.1
    logits[2 * p:, 0] = 30.0                                                     # no foreground in image 2
    bbox = torch.randn(b * p, c, 4, generator=g) * 0.3
    n0, n1 = int(s["counts"][0]), int(s["counts"][1])
    poisoned = [0, 1, n0 // 2, n0 - 1, p + 0, p + 3, p + n1 - 1]
    for i, r in enumerate(poisoned):
        _poison(logits[r], NONFINITE_KINDS[i % 4], g)
        bbox[r] = float("nan")
    windows = torch.tensor([[0., 0., 1024., 1024.], [128., 0., 896., 1024.], [0., 0., 1024., 1024.]])
    ns = SimpleNamespace(cfg=s["cfg"])
    args = (s["rois"].to(dev), s["counts"].to(dev), logits.to(dev), bbox.to(dev), windows.to(dev))
    ids, scores, boxes, nrois, kept = (t.cpu() for t in MaskRCNNInference.detections(ns, *args))
    assert not torch.isnan(scores).any() and not torch.isnan(boxes).any()
    dets, nms_cls, class_ids = (t.cpu() for t in ops.detection_decode(args[2], args[3], args[0], args[1], args[4], STD, 1024, 1024, 0.0))
    for r in poisoned:
        assert int(nms_cls.view(-1)[r]) == -(r % p + 1) and int(class_ids.view(-1)[r]) == 0      # absent on the HIP side
    total = 0
    for i in range(b):
        n, k = int(s["counts"][i]), int(kept[i])
        probs = torch.softmax(logits[i * p:i * p + n], dim=1)
        bad = [r - i * p for r in poisoned if i * p <= r < i * p + n]
        assert all(bool(torch.isnan(probs[r]).all()) and int(torch.max(probs[r], 0)[1]) == 0 for r in bad)   # absent in the reference
        cls, sc, bx = oracle.mrn_refine(s["rois"][i, :n], probs, bbox[i * p:i * p + n], tuple(windows[i].tolist()), ocfg)
        assert not ids[i, k:].any() and not scores[i, k:].any() and not boxes[i, k:].any()
        if cls is None:
            assert k == 0
            continue
        assert i != 2 and k == cls.size(1) and not torch.isnan(sc).any()
        total += k
        key = lambda c_, b_: [tuple(v) for v in torch.cat([c_.view(-1, 1).double(), b_.double()], 1).tolist()]
        mine, ref = key(ids[i, :k], boxes[i, :k]), key(cls[0], bx[0])
        assert len(set(mine)) == k and set(mine) == set(ref)
        ref_score = dict(zip(ref, sc[0].tolist()))
        assert max(abs(ref_score[m] - v) for m, v in zip(mine, scores[i, :k].tolist())) <= 1e-6
        # exactly, in order, from the dets the HIP path used
        valid = (nms_cls[i] > 0).nonzero().flatten()
        survivors = valid[oracle.nms(dets[i][valid], ocfg.DETECTION_NMS_THRESHOLD, class_ids=nms_cls[i][valid])]
        order = survivors[torch.sort(dets[i][survivors, 4], descending=True, stable=True).indices]
        assert order.numel() == k
        assert torch.equal(ids[i, :k], class_ids[i][order]) and torch.equal(boxes[i, :k], dets[i][order, :4])
        assert torch.equal(scores[i, :k], dets[i][order, 4]) and torch.equal(nrois[i, :k], dets[i][order, :4] / 1024.0)
    assert total > 100 and int(kept[2]) == 0
    assert int((scores == 1.0).sum()) > 50                                        # saturated winners survive as exact ties
    cfg50, _ = _stage_cfgs(oracle, 50)
    ids50, scores50, boxes50, _, kept50 = (t.cpu() for t in MaskRCNNInference.detections(SimpleNamespace(cfg=cfg50), *args))
    assert kept50.tolist() == [min(int(v), 50) for v in kept]
    assert torch.equal(ids50, ids[:, :50]) and torch.equal(scores50, scores[:, :50]) and torch.equal(boxes50, boxes[:, :50])


# ==================================================================================== pyramid RoIAlign side paths
def _roi_align(fms, rois, roi_batch, rois_per_image, roi_counts, pool, area, layout, dev, num_rois=None):
    """fms: four NHWC device tensors. layout 0 = NHWC, 1 = k-blocked, 2 = NHWC fp16. → (guarded output, levels)."""
    from maskrcnn_amd._lib import c_i32, c_vp, lib
    b, _, _, depth = fms[0].shape
    r = rois.size(0) if num_rois is None else num_rois
    shape = (depth // 8, r * pool * pool, 8) if layout == 1 else (r, pool, pool, depth)
    out = _Out(shape, torch.float16 if layout == 2 else F32, dev)
    levels = _Out((r,), I32, dev)
    rd = rois.to(dev).contiguous()
    rb = None if roi_batch is None else roi_batch.to(dev)
    rc = None if roi_counts is None else roi_counts.to(dev)
    _run(lib.mrcnn_roi_align_pyramid_counted_f32,
         (_arr(c_vp, [f.data_ptr() for f in fms]), _arr(c_i32, [f.size(1) for f in fms]), _arr(c_i32, [f.size(2) for f in fms]),
          b, depth, rd.data_ptr(), None if rb is None else rb.data_ptr(), r, rois_per_image,
          None if rc is None else rc.data_ptr(), pool, float(area), out.ptr, layout, levels.ptr), (out, levels))
    return out, levels.t.cpu()


def _as_nhwc(out, layout, r, pool, depth):
    t = out.t.cpu()
    if layout == 1:
        return t.permute(1, 0, 2).reshape(r, pool, pool, depth)
    return t


def _rand_rois(g, n):
    c = torch.rand(n, 2, generator=g) * 0.8 + 0.1
    hw = torch.exp(torch.rand(n, 2, generator=g) * 3.2 - 3.6)                      # 0.027 .. 0.67: all four levels
    return torch.cat([c - hw / 2, c + hw / 2], 1).clamp(0, 1)


@pytest.mark.parametrize("depth", [4, 260, 512])
def test_roi_align_pyramid_roi_batch_counts_layouts_and_pool_1(dev, oracle, depth):
    """The side paths of mrcnn_roi_align_pyramid_counted_f32 at depth 4 (one lane), 260 (a second 256-channel step of one lane)
    and 512: an explicit roi_batch in shuffled order with two out-of-range indices (rows of zeros); roi_counts of 0, 1 and all
    (rows past the count keep the guard pattern) in all three output layouts; pool 1 (box centre computed in double) and 7;
    num_rois == 0 (nothing written). Live rows bit for bit against oracle.roi_align."""
    g = torch.Generator().manual_seed(7100 + depth)
    b, shape, rpi = 3, (1024, 1024, 3), 8       # the image shape only selects the level: the maps are small and not square
    area = float(shape[0] * shape[1])
    nchw = [torch.randn(b, depth, 128 // s, 160 // s, generator=g) for s in (4, 8, 16, 32)]
    fms = [f.permute(0, 2, 3, 1).contiguous().to(dev) for f in nchw]
    layouts = (0, 2) if depth % 8 else (0, 1, 2)
    r = b * rpi
    rois = _rand_rois(g, r)
    for i, side in enumerate((0.03, 0.15, 0.3, 0.8)):                              # one box of each level for certain
        rois[i] = torch.tensor([0.5 - side / 2, 0.5 - side / 2, 0.5 + side / 2, 0.5 + side / 2])
    want_levels = oracle.roi_levels(rois, shape)
    assert set(want_levels.tolist()) == {2, 3, 4, 5}

    def want_rows(pool, image_of):
        w = torch.zeros(r, pool, pool, depth)
        for i in range(b):
            ix = (image_of == i).nonzero().flatten()
            if ix.numel():
                w[ix] = oracle.roi_align(rois[ix], [f[i:i + 1] for f in nchw], pool, shape).permute(0, 2, 3, 1)
        return w

    for pool in (1, 7):
        # explicit roi_batch
        rb = torch.randint(0, b, (r,), generator=g, dtype=I32)
        rb[5], rb[17] = -1, b
        want = want_rows(pool, rb)
        for layout in layouts:
            out, levels = _roi_align(fms, rois, rb, 0, None, pool, area, layout, dev)
            got = _as_nhwc(out, layout, r, pool, depth)
            assert torch.equal(levels, want_levels)
            assert torch.equal(got.float(), want.half().float() if layout == 2 else want), (depth, pool, layout)
            assert not got[5].any() and not got[17].any()
        # roi_counts
        counts = torch.tensor([0, 1, rpi], dtype=I32)
        image_of = torch.arange(r) // rpi
        live = (torch.arange(r) % rpi) < counts[image_of]
        want = want_rows(pool, torch.where(live, image_of, torch.full_like(image_of, -1)))
        for layout in layouts:
            out, levels = _roi_align(fms, rois, None, rpi, counts, pool, area, layout, dev)
            got = _as_nhwc(out, layout, r, pool, depth)
            assert torch.equal(got[live].float(), (want.half().float() if layout == 2 else want)[live]), (depth, pool, layout)
            assert bool((got[~live] == 7).all()) and bool((levels[~live] == 7).all()), (depth, pool, layout)
            assert torch.equal(levels[live], want_levels[live])
    out, _ = _roi_align(fms, rois, None, rpi, None, 7, area, 0, dev, num_rois=0)      # the bands are the whole buffer
    assert out.n == 0 and bool((out.buf == 7).all())


# ================================================================================================= crop_backward
def _crop_backward(grads, boxes, index, batch, depth, h, w, dev):
    from maskrcnn_amd._lib import lib
    n, _, ch, cw = grads.shape
    gi = _Out((batch, depth, h, w), F32, dev)
    gi.t.fill_(3.0)                                                               # must be zeroed by the callee
    gd, bd, ix = grads.contiguous().to(dev), boxes.contiguous().to(dev), index.to(dev)
    _run(lib.mrcnn_crop_backward_f32, (gd.data_ptr() if n else None, bd.data_ptr() if n else None, ix.data_ptr() if n else None,
                                       n, batch, depth, h, w, ch, cw, gi.ptr), (gi,))
    return gi.t.cpu()


def _samples_f32(c1, c2, size, crop):
    """The sample positions of crop_and_resize (crop_cpu.cpp:52-61) in fp32, op for op → (inside, lo, hi, lerp) per crop row."""
    f = np.float32
    t = np.arange(crop, dtype=np.float32)
    if crop > 1:
        scale = f(f(f(c2) - f(c1)) * f(size - 1)) / f(crop - 1)
        pos = f(c1) * f(size - 1) + t * scale
    else:
        pos = np.array([f(0.5 * float(f(c1) + f(c2)) * float(size - 1))], dtype=np.float32)
    inside = ~((pos < 0) | (pos > f(size - 1)))
    lo, hi = np.floor(pos).astype(np.int64), np.ceil(pos).astype(np.int64)
    return inside, lo, hi, (pos - lo.astype(np.float32)).astype(np.float32)


def _crop_backward_ref(grads, boxes, index, batch, depth, h, w):
    """float64 accumulation of the terms crop_backward adds (crop_cpu.cpp:244-260), with the sample positions and the four
    bilinear weights as the fp32 values the kernel holds. → (sum, sum of |term|, number of terms) per image element."""
    n, _, ch, cw = grads.shape
    tot, mag = np.zeros((batch, depth, h, w)), np.zeros((batch, depth, h, w))
    cnt = np.zeros((batch, h, w), dtype=np.int64)
    g64 = grads.double().numpy()
    for i in range(n):
        bi = int(index[i])
        if bi < 0 or bi >= batch:
            continue
        iy, ylo, yhi, yl = _samples_f32(*boxes[i, [0, 2]].tolist(), h, ch)
        ix, xlo, xhi, xl = _samples_f32(*boxes[i, [1, 3]].tolist(), w, cw)
        for (ys, yw) in ((ylo, (np.float32(1) - yl).astype(np.float64)), (yhi, yl.astype(np.float64))):
            for (xs, xw) in ((xlo, (np.float32(1) - xl).astype(np.float64)), (xhi, xl.astype(np.float64))):
                for r in np.nonzero(iy)[0]:
                    for q in np.nonzero(ix)[0]:
                        term = g64[i, :, r, q] * (yw[r] * xw[q])
                        tot[bi, :, ys[r], xs[q]] += term
                        mag[bi, :, ys[r], xs[q]] += np.abs(term)
                        cnt[bi, ys[r], xs[q]] += 1
    return tot, mag, cnt


def _assert_crop_backward(got, ref, tag):
    """|got - float64 sum| <= n_terms * 2^-23 * sum|term| per element: the fp32 summation's own bound. A term omx * (omy * g) is
    two rounded products of the fp32 weights (2 * 2^-24 of |term|), and adding n terms in any order rounds at most n - 1 times
    (2^-24 each, of a partial sum no larger than sum|term|): (n + 1) * 2^-24 <= n * 2^-23, tight for a single term. Elements
    no term reaches must be exactly zero."""
    tot, mag, cnt = ref
    bound = cnt[:, None].astype(np.float64) * 2.0 ** -23 * mag
    err = np.abs(got.double().numpy() - tot)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"crop_backward {tag}: up to {int(cnt.max())} terms per pixel, max err {err.max():.3e}, worst err / bound {worst:.3f}")
    assert (err <= bound).all(), tag
    return int(cnt.max())


def test_crop_backward_piled_boxes_slabs_and_side_paths(dev):
    """(a) 500 boxes piled onto one 8 x 8 region: hundreds of atomic terms per pixel, against the float64 sum within the
    summation's own bound n_terms * 2^-23 * sum|term| (measured: at most 0.063 of it). (b) depth * crop_h * crop_w > 8192:
    several channel slabs per box. (c) 1 x 1 crops. (d) boxes wholly outside the image and out-of-range box_index: no
    contribution. (e) num_boxes == 0 still zeroes grads_image."""
    g = torch.Generator().manual_seed(8100)
    # (a)
    batch, depth, h, w, n = 2, 3, 24, 20, 500
    tl = torch.tensor([8.0 / (h - 1), 6.0 / (w - 1)]) + torch.rand(n, 2, generator=g) * 0.02
    boxes = torch.cat([tl, tl + torch.tensor([7.0 / (h - 1), 7.0 / (w - 1)]) * (0.6 + 0.4 * torch.rand(n, 2, generator=g))], 1)
    index = torch.ones(n, dtype=I32)
    grads = torch.randn(n, depth, 4, 4, generator=g)
    got = _crop_backward(grads, boxes, index, batch, depth, h, w, dev)
    assert _assert_crop_backward(got, _crop_backward_ref(grads, boxes, index, batch, depth, h, w), "piled") >= 300
    assert not got[0].any()
    # (b) 40 channels x 15 x 15 = 9000 > 8192, boxes spilling over the border, reversed, a bad index, a box outside
    batch, depth, h, w, n = 2, 40, 18, 22, 12
    c = torch.rand(n, 2, generator=g)
    hw = torch.rand(n, 2, generator=g) * 0.7 + 0.05
    boxes = torch.cat([c - hw / 2, c + hw / 2], 1)
    boxes[1] = torch.tensor([0.8, 0.9, 0.2, 0.1])
    boxes[2] = torch.tensor([-0.6, -0.5, -0.1, -0.2])                             # wholly outside: nothing
    boxes[3] = torch.tensor([1.2, 0.1, 1.9, 0.5])
    index = torch.randint(0, batch, (n,), generator=g, dtype=I32)
    index[4], index[5] = -1, batch                                                # out of range: nothing, and no fault
    grads = torch.randn(n, depth, 15, 15, generator=g)
    ref = _crop_backward_ref(grads, boxes, index, batch, depth, h, w)
    got = _crop_backward(grads, boxes, index, batch, depth, h, w, dev)
    _assert_crop_backward(got, ref, "slabs")
    only = torch.tensor([2, 3, 4, 5])
    assert not _crop_backward(grads[only], boxes[only], index[only], batch, depth, h, w, dev).any()
    # (c)
    grads = torch.randn(n, depth, 1, 1, generator=g)
    got = _crop_backward(grads, boxes, index, batch, depth, h, w, dev)
    _assert_crop_backward(got, _crop_backward_ref(grads, boxes, index, batch, depth, h, w), "1x1")
    assert got.any()
    # (e)
    assert not _crop_backward(torch.zeros(0, depth, 7, 7), torch.zeros(0, 4), torch.zeros(0, dtype=I32), batch, depth, h, w, dev).any()
