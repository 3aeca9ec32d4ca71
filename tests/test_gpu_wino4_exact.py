"""GPU sweep (-m gpu) of the Winograd F(4x4) kernels of csrc/conv_wino4.hip on exact data (tests/wino4_exact_cases.py; the twin
of tests/test_gpu_fused_exact.py): the plain conv, the form with the RPN heads, the form with the Bottleneck's conv3, and the
filter transform. The conv kernels take the transformed filter U as an operand, so they are handed a synthetic U of small
integers with one non-zero component per output channel: the bilinear form Y = A^T [sum_c U_c .* (B^T d_c B)] A is then exact
in fp32 in any order, and each kernel must equal a float64 evaluation of it BIT FOR BIT. Every operand sits between NaN bands
(U is moved between bands of its own once more) and every output between 0xFF bands (the outputs go to the C entry points, as the
bindings allocate their own); a second call gives the same bits; image i of a batch equals image i alone; the k-blocked output
equals the NHWC output re-blocked. The last test runs the file once more on the schedule-fuzzing build.

Signed zeros: the reference's +0 is required everywhere, with and without ReLU. No instruction of these kernels produces -0 from
these data: the plain epilogue ends in v_pk_fma_f32(y, scale, shift) — with no scale and shift vectors its operands are 1 and +0
—, and in round-to-nearest a sum is -0 only if both addends are, while every shift here is +0 or non-zero; the MFMAs of the heads
and of conv3 start from +0 accumulators, and conv3's last instruction is v_max_f32 0, x.

The filter transform: bit equality on g = 3^10 * {-2..2} * 2^k, whose U is a short integer (an exact zero may be -0: the double
division by a negative N_p produces it, see the test); on random fp32 g at most one fp32 ulp
from the exact rational value rounded once (the kernel rounds twice: double arithmetic, then the cast)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wino4_exact_cases as C
from test_gpu_conv_exact import _banded, _bands_intact, _bits, _poisoned  # noqa: F401
from test_gpu_fused_exact import FUZZ_LIB, ROOT, _assert_bits, _exact, _p, _rebanded, _stream

pytestmark = pytest.mark.gpu
F32 = torch.float32
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
CASES = C.cases(CUS)
_ID = lambda v: v.id if hasattr(v, "id") else v


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import maskrcnn_amd  # noqa: F401
    return torch.device("cuda:0")


def _conv_operands(d, dev, images=None):
    """x k-blocked (the whole batch, or image i alone), U in the kernel's layout, scale, shift."""
    x = d.x if images is None else d.x[images:images + 1]
    return (_banded(C.kblocked(x), F32, dev), _rebanded(_banded(C.u_layout(d.u), F32, dev)), _banded(d.scale, F32, dev),
            _banded(d.shift, F32, dev))


# ---------------------------------------------------------------------------------------------------------------------
# plain
# ---------------------------------------------------------------------------------------------------------------------
PLAIN_RUNS = [(c, out) for c in CASES if c.form == "plain" for out in (("both",) if c.tag else ("nhwc", "kblocked", "both"))]


def run_plain(dev, case, out, wants):
    """One case and output form through all four (scale and shift, ReLU) variants against `wants[variant]` (NHWC)."""
    from maskrcnn_amd._lib import check, lib
    d = C.build(case)
    b, h, w, cin, cout = case.b, case.h, case.w, case.cin, case.cout
    assert int(lib.mrcnn_conv3x3_winograd4_supported(b, h, w, cin, cout)) == 1
    x, u, scale, shift = _conv_operands(d, dev)
    ones = [_conv_operands(d, dev, i)[0] for i in range(b)] if b > 1 else []
    nhwc, kb = out != "kblocked", out != "nhwc"

    def shapes(n):
        return ([(n, h, w, cout)] if nhwc else []) + ([(cout // 8, n, h, w, 8)] if kb else [])

    def launch(xt, n, with_scale, with_relu):
        def go(outs):
            y, yk = (outs[0] if nhwc else None), (outs[-1] if kb else None)
            check(lib.mrcnn_conv3x3_winograd4_f32(xt.data_ptr(), n, h, w, cin, u.data_ptr(), cout, _p(scale if with_scale else None),
                                                  _p(shift if with_scale else None), int(with_relu), _p(y), _p(yk), _stream()))
        return go

    for with_scale, with_relu in C.VARIANTS:
        want = wants[(with_scale, with_relu)]
        ws = ([want] if nhwc else []) + ([C.kblocked(want)] if kb else [])
        what = f"{case.id} ->{out} scale={with_scale} relu={with_relu}"
        got = _exact(what, dev, launch(x, b, with_scale, with_relu), shapes(b), F32, ws)
        if out == "both":
            from maskrcnn_amd import ops
            assert torch.equal(_bits(ops.nhwc_to_kblocked(got[0])), _bits(got[1])), f"{what}: k-blocked != NHWC re-blocked"
        for i, xi in enumerate(ones):
            one = _exact(f"{what} image {i}", dev, launch(xi, 1, with_scale, with_relu), shapes(1), F32, [None] * len(ws))
            for o1, whole in zip(one, got):
                part = whole[i:i + 1] if whole.dim() == 4 else whole[:, i:i + 1]
                assert torch.equal(_bits(o1), _bits(part)), f"{what}: image {i} alone differs from image {i} of the batch"


@pytest.mark.parametrize("case,out", PLAIN_RUNS, ids=_ID)
def test_winograd_f4x4_is_exact(dev, case, out):
    """mrcnn_conv3x3_winograd4_f32: a single position, one M tile, ragged blocks with a wrapping k ring and two N tiles, four N
    tiles, three images, one row of M tiles past the persistent-grid clamp; outputs NHWC, k-blocked and both; ReLU on and off;
    scale and shift present and null."""
    run_plain(dev, case, out, C.build(case).want)


# ---------------------------------------------------------------------------------------------------------------------
# the RPN heads inside the conv
# ---------------------------------------------------------------------------------------------------------------------
def run_heads(dev, case, want):
    """`want`: (the raw M-tile-major rows [tiles * 512, 32], to_nhwc(bias) [B,H,W,18])."""
    from maskrcnn_amd._binding import HeadSums
    from maskrcnn_amd._lib import check, lib
    d = C.build(case)
    b, h, w, cin, cout = case.b, case.h, case.w, case.cin, case.cout
    x, u, scale, shift = _conv_operands(d, dev)
    wh, bias = _banded(d.w_head32, F32, dev), _banded(d.bias, F32, dev)
    rows = lambda n: int(lib.mrcnn_conv3x3_winograd4_heads_rows(n, h, w))
    assert rows(b) == want[0].shape[0] and rows(b) == b * rows(1)

    def launch(xt, n):
        return lambda outs: check(lib.mrcnn_conv3x3_winograd4_heads_f32(
            xt.data_ptr(), n, h, w, cin, u.data_ptr(), cout, scale.data_ptr(), shift.data_ptr(), 1, wh.data_ptr(),
            outs[0].data_ptr(), _stream()))

    # every row, those of positions outside the image included: the kernel stages zeros beyond the image and stores all 512
    # rows of an M tile, so they hold the form on the zero-extended image — as the reference computes them
    part, = _exact(case.id, dev, launch(x, b), [(rows(b), 32)], F32, [want[0]])
    assert not bool(_bits(part[:, 18:]).any()), f"{case.id}: a padded head column is not +0"
    _assert_bits(HeadSums(part, b, h, w, 3).to_nhwc(bias), want[1], dev, f"{case.id} to_nhwc")
    if b > 1:
        for i in range(b):
            p1, = _exact(f"{case.id} image {i}", dev, launch(_conv_operands(d, dev, i)[0], 1), [(rows(1), 32)], F32, [None])
            assert torch.equal(_bits(p1), _bits(part[i * rows(1):(i + 1) * rows(1)])), \
                f"{case.id}: image {i} alone differs from image {i} of the batch"


@pytest.mark.parametrize("case", [c for c in CASES if c.form == "heads"], ids=_ID)
def test_rpn_heads_inside_the_f4x4_conv_are_exact(dev, case):
    """mrcnn_conv3x3_winograd4_heads_f32: every real head row sums two or more conv channels of at least two N tiles (the sums
    wait in LDS through the N-tile walk), two and four N tiles, 18 M tiles in one image (walks that start at N tile 1), one row
    of M tiles past the clamp. The raw rows — 14 zero columns, rows of positions outside the image — and to_nhwc(bias)."""
    run_heads(dev, case, C.build(case).want[(True, True)])


# ---------------------------------------------------------------------------------------------------------------------
# conv2 + conv3
# ---------------------------------------------------------------------------------------------------------------------
def run_conv3(dev, case, wants):
    from maskrcnn_amd._lib import check, lib
    d = C.build(case)
    b, h, w, cin, c3 = case.b, case.h, case.w, case.cin, case.c3
    x, u, scale, shift = _conv_operands(d, dev)
    w3, s3, t3 = _banded(d.w3, F32, dev), _banded(d.scale3, F32, dev), _banded(d.shift3, F32, dev)
    res = _banded(d.residual, F32, dev)

    def launch(xt, rt, n, affine3):
        return lambda outs: check(lib.mrcnn_conv3x3_winograd4_conv3_f32(
            xt.data_ptr(), n, h, w, cin, u.data_ptr(), scale.data_ptr(), shift.data_ptr(), w3.data_ptr(), c3,
            _p(s3 if affine3 else None), _p(t3 if affine3 else None), rt.data_ptr(), outs[0].data_ptr(), _stream()))

    for affine3 in (True, False):
        what = f"{case.id} scale3/shift3={affine3}"
        got, = _exact(what, dev, launch(x, res, b, affine3), [(b, h, w, c3)], F32, [wants[(affine3, True)]])
        if b > 1:
            for i in range(b):
                xi, ri = _conv_operands(d, dev, i)[0], _banded(d.residual[i:i + 1], F32, dev)
                one, = _exact(f"{what} image {i}", dev, launch(xi, ri, 1, affine3), [(1, h, w, c3)], F32, [None])
                assert torch.equal(_bits(one), _bits(got[i:i + 1])), f"{what}: image {i} alone differs from image {i} of the batch"


@pytest.mark.parametrize("case", [c for c in CASES if c.form == "conv3"], ids=_ID)
def test_f4x4_conv2_with_conv3_is_exact(dev, case):
    """mrcnn_conv3x3_winograd4_conv3_f32: c3 32 / 96 / 256 (one, three, eight column blocks of W3 resident in LDS), one M tile,
    ragged 5 x 11 positions, two single-position images; scale3 / shift3 present and null; the residual added before the ReLU."""
    run_conv3(dev, case, C.build(case).want)


def test_the_case_table_is_complete():
    assert C.coverage_problems(CASES) == []


# ---------------------------------------------------------------------------------------------------------------------
# the filter transform
# ---------------------------------------------------------------------------------------------------------------------
def _transform(dev, g, what, want):
    from maskrcnn_amd._lib import check, lib
    cout, cin = g.shape[0], g.shape[3]
    wt = _banded(g, F32, dev)
    u, = _exact(what, dev, lambda outs: check(lib.mrcnn_winograd4_weights_f32(wt.data_ptr(), cout, cin, outs[0].data_ptr(), _stream())),
                [(cin // 4, 36, 2, cout, 2)], F32, [want])
    return u


@pytest.mark.parametrize("cout,cin", C.WEIGHT_SHAPES)
def test_filter_transform_is_exact_on_3_to_the_10_data(dev, cout, cin):
    """Bit equality wherever the exact value is not zero. An exact zero may carry either sign: the kernel evaluates a row of G
    as (x0 + p x1 + p^2 x2) / N_p in double, N_+3/4 and N_-3/4 are negative (-243/128), and that division turns a numerator of +0
    (a zero tap column, a cancelling sum) into -0, which the cast keeps. In the conv kernels a -0 entry of U adds +-0 to an
    accumulator that starts at +0: no bit of any output depends on it."""
    g, u = C.weights_int(cout, cin)
    want = C.u_layout(u).astype(np.float32)
    got = _transform(dev, g, f"winograd4_weights {cout}x{cin}", None)
    zero = torch.from_numpy(want == 0).to(dev)
    assert not bool(got[zero].any()), f"winograd4_weights {cout}x{cin}: a non-zero value where the exact value is 0"
    _assert_bits(torch.where(zero, torch.zeros_like(got), got), want, dev, f"winograd4_weights {cout}x{cin}")


@pytest.mark.parametrize("cout,cin", C.WEIGHT_REAL_SHAPES)
def test_filter_transform_within_one_ulp_on_real_data(dev, cout, cin):
    g, u = C.weights_real(cout, cin)
    want = torch.from_numpy(C.u_layout(u)).to(dev)
    got = _transform(dev, g, f"winograd4_weights real {cout}x{cin}", None)
    ulps = (_bits(got).long() - _bits(want).long()).abs()      # same sign wherever they differ by an ulp: no value here is near 0
    differ = float((ulps != 0).float().mean())
    print(f"\nwinograd4_weights {cout}x{cin}: {differ:.5f} of the elements differ from the once-rounded exact value, max {int(ulps.max())} ulp")
    assert int(ulps.max()) <= 1, (cout, cin, int(ulps.max()))


# ---------------------------------------------------------------------------------------------------------- schedule fuzzing
# The child's time limit: four times the wall time measured on the fuzzed library, rounded up to the next 10 s: 5.8 s for the
# first 32 of its 38 tests (4.2 s of it inside pytest, the rest start-up; the remaining six take 1.5 s on the plain library),
# so 7.3 s, 4 x 7.3 = 29.2 -> 30 s.
FUZZ_TIMEOUT = 30


@pytest.mark.skipif(os.environ.get("MRCNN_SYNC_FUZZ_CHILD") == "1", reason="this IS the fuzzed child run")
def test_this_file_passes_under_schedule_fuzzing():
    """The F(4x4) kernels place every barrier by hand (s_waitcnt + s_barrier pairs around the staging ring, the exchange
    buffer that aliases it, the heads' sums in LDS, conv3's tile inside the exchange buffer). On the schedule-fuzzing build every
    wave sleeps a random time behind each barrier: a hand-off that a barrier does not order gives other bits there, and every
    comparison above is a comparison of bits."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_wino4_exact.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=FUZZ_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
