"""GPU sweep (-m gpu) of the implicit-GEMM convs on exact data (tests/conv_exact_cases.py): small integers times powers of two,
for which every product and partial sum is exact in fp32, so the kernels must equal a float64 evaluation BIT FOR BIT in any
summation order. Every operand and the output sit between guard bands (NaN around the operands, 0xFF bytes around the output).

What this proves is indexing: rows, columns, taps, padding, tails, images, epilogues, layouts and the fp16 conversions. It does
not measure accumulation accuracy on real-valued data: that stays with the tolerance tests of tests/test_gpu_conv.py."""
import numpy as np
import pytest
import torch

import conv_exact_cases as C
from test_conv_exact_host import coverage_problems

pytestmark = pytest.mark.gpu
TOL = 1e-4       # tests/test_gpu_conv.py's bar; here it covers the sigmoid function only (its argument is exact)
BAND = 1024      # elements of guard band on either side of every tensor

CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
FP32_CASES = C.fp32_cases(CUS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import maskrcnn_amd  # noqa: F401
    return torch.device("cuda:0")


def _banded(a, dtype, dev):
    """The array as a contiguous slice of a larger device buffer whose surroundings hold NaN."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    buf = torch.full((t.numel() + 2 * BAND,), float("nan"), dtype=dtype, device=dev)
    buf[BAND:BAND + t.numel()] = t.reshape(-1).to(dev)
    return buf[BAND:BAND + t.numel()].view(t.shape)


def _poisoned(shape, dtype, dev):
    """An output of this shape between two bands, every byte 0xFF (a NaN in either float type). -> (whole buffer, output)"""
    size = torch.empty(0, dtype=dtype).element_size()
    n = int(np.prod(shape))
    buf = torch.full(((n + 2 * BAND) * size,), 0xFF, dtype=torch.uint8, device=dev)
    return buf, buf[BAND * size:(BAND + n) * size].view(dtype).view(*shape)


def _bands_intact(buf, out):
    lo = BAND * out.element_size()
    return bool((buf[:lo] == 0xFF).all()) and bool((buf[lo + out.numel() * out.element_size():] == 0xFF).all())


def _out_shape(case, b=None):
    b = case.b if b is None else b
    oh, ow = case.out_hw
    return {0: (b, oh, ow, case.cout), 1: (b, 2 * oh, 2 * ow, case.cout // 4), 2: (case.cout // 8, b, oh, ow, 8)}[case.out_mode]


def _operands(case, d, dev):
    """Device tensors of the case, each between NaN bands, in the types the entry point reads."""
    xt = torch.float16 if case.x16 else torch.float32
    rt = torch.float16 if case.y16 else torch.float32
    t = {"x": _banded(d.x, xt, dev), "scale": None if d.scale is None else _banded(d.scale, torch.float32, dev),
         "shift": _banded(d.shift, torch.float32, dev), "residual": None, "w_lo": None}
    if d.residual is not None:
        t["residual"] = _banded(C.kblocked(d.residual) if case.res_kblocked else d.residual, rt, dev)
    if case.op == "f32":
        t["w"] = _banded(d.w, torch.float32, dev)
    elif case.products == 3:
        w32 = torch.from_numpy(d.w).float()
        hi = w32.half()
        t["w"], t["w_lo"] = _banded(hi.numpy(), torch.float16, dev), _banded((w32 - hi.float()).numpy(), torch.float16, dev)
    else:
        t["w"] = _banded(d.w, torch.float16, dev)
    if case.rows:
        t["row_counts"] = torch.tensor(case.rows[1], dtype=torch.int32, device=dev)
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch(case, t, out, b=None, out32=None):
    """One call of the case's entry point on `b` images (default: all) into `out`."""
    from maskrcnn_amd import ops
    from maskrcnn_amd._lib import check, lib
    b = case.b if b is None else b
    s = torch.cuda.current_stream().cuda_stream
    x, w, k = t["x"], t["w"], case.k
    geom = (b, case.h, case.w, case.cin)
    taps = (case.cout, k, k, case.stride, *case.pad)
    aff = (_ptr(t["scale"]), _ptr(t["shift"]))
    if case.op == "f32":
        if case.out_mode == 1:
            check(lib.mrcnn_deconv2x2_bias_act_nhwc_f32(x.data_ptr(), *geom, w.data_ptr(), case.cout // 4, aff[1], case.act,
                                                        out.data_ptr(), s))
        elif case.out_mode == 2:
            check(lib.mrcnn_conv_bn_act_f32(x.data_ptr(), *geom, w.data_ptr(), *taps, *aff, _ptr(t["residual"]), max(case.res, 1),
                                            int(case.res_kblocked), case.act, out.data_ptr(), 1, s))
        else:
            rows = dict(row_counts=t["row_counts"], rows_per_group=case.rows[0]) if case.rows else {}
            got = ops.conv_bn_act(x, w, t["scale"], t["shift"], case.stride, case.pad, case.act, t["residual"], max(case.res, 1),
                                  out=out, **rows)
            assert got.data_ptr() == out.data_ptr()
    elif case.op == "f16mfma":
        if case.out_mode == 1:
            check(lib.mrcnn_deconv2x2_bias_act_nhwc_f16mfma(x.data_ptr(), *geom, w.data_ptr(), _ptr(t["w_lo"]), case.cout // 4,
                                                            aff[1], case.act, case.products, out.data_ptr(), s))
        else:
            check(lib.mrcnn_conv_bn_act_nhwc_f16mfma(x.data_ptr(), *geom, w.data_ptr(), _ptr(t["w_lo"]), *taps, *aff,
                                                     _ptr(t["residual"]), max(case.res, 1), case.act, case.products,
                                                     out.data_ptr(), s))
    elif case.op == "f16io":
        if case.out_mode == 1:
            check(lib.mrcnn_deconv2x2_bias_act_nhwc_f16io(x.data_ptr(), *geom, w.data_ptr(), case.cout // 4, aff[1], case.act,
                                                          out.data_ptr(), s))
        else:
            check(lib.mrcnn_conv_bn_act_nhwc_f16io(x.data_ptr(), int(case.x16), *geom, w.data_ptr(), *taps, *aff,
                                                   _ptr(t["residual"]), max(case.res, 1), case.act, out.data_ptr(), int(case.y16), s))
    else:
        check(lib.mrcnn_conv_f16_pipelined(x.data_ptr(), *geom, w.data_ptr(), *taps, *aff, _ptr(t["residual"]), max(case.res, 1),
                                           case.act, out.data_ptr(), _ptr(out32), *case.tile, s))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _image(case, t, i):
    """The operands of image i alone."""
    one = dict(t)
    one["x"] = t["x"][i:i + 1]
    if t["residual"] is not None:
        one["residual"] = t["residual"][:, i:i + 1].contiguous() if case.res_kblocked else t["residual"][i:i + 1]
    return one


def _live_rows(case, bm):
    """Mask of the output rows in M tiles that hold a valid row (conv_common.hpp tile_has_rows, through ops.rows_executed's
    rule: valid rows are a prefix of every group)."""
    per, counts = case.rows
    valid = np.zeros(case.m, bool)
    for g, n in enumerate(counts):
        valid[g * per:g * per + n] = True
    live = np.zeros(case.m, bool)
    for m0 in range(0, case.m, bm):
        live[m0:m0 + bm] = valid[m0:m0 + bm].any()
    return live


def _check_sigmoid(case, d, got):
    """The argument of the sigmoid is exact: outputs with one argument hold one bit pattern, and the outputs are
    non-decreasing in the argument — both exact. The values themselves are held to TOL against float64."""
    pre = d.pre.reshape(-1)
    y = got.reshape(-1).double().cpu().numpy()
    order = np.argsort(pre, kind="stable")
    ps, ys = pre[order], y[order]
    same = ps[1:] == ps[:-1]
    assert np.array_equal(ys[1:][same], ys[:-1][same]), f"{case.id}: one pre-activation, two outputs"
    assert bool((ys[1:] >= ys[:-1]).all()), f"{case.id}: the outputs are not monotonic in the exact pre-activation"
    err = float(np.abs(y - d.want.reshape(-1)).max())
    assert err <= TOL, f"{case.id}: sigmoid off by {err:.3e}"


def _run_exact(case, dev):
    from maskrcnn_amd import ops
    d = C.build(case)
    C.check_invariants(case, d)
    t = _operands(case, d, dev)
    ydt = torch.float16 if case.y16 else torch.float32
    buf, out = _poisoned(_out_shape(case), ydt, dev)
    buf32 = out32 = None
    if case.op == "f16p":    # both outputs of the pipelined kernel
        buf32, out32 = _poisoned(_out_shape(case), torch.float32, dev)
    _launch(case, t, out, out32=out32)
    torch.cuda.synchronize()
    assert _bands_intact(buf, out), f"{case.id}: a byte of the output's guard bands changed"
    first = out.clone()
    if case.act == 2:
        _check_sigmoid(case, d, first)
    else:
        want = torch.from_numpy(d.want.astype(np.float16 if case.y16 else np.float32)).to(dev)
        if case.rows:
            live = torch.from_numpy(_live_rows(case, int(ops.lib.mrcnn_conv_rows_tile_m(case.cout)))).to(dev)
            g, wnt = _bits(first).view(case.m, case.cout), _bits(want).view(case.m, case.cout)
            assert torch.equal(g[live], wnt[live]), f"{case.id}: rows of live tiles differ"
            assert bool((g[~live] == -1).all()), f"{case.id}: a skipped tile wrote to its rows"
            assert 0 < int(live.sum()) < case.m
        else:
            bad = _bits(first) != _bits(want)     # as bits: +0 where the reference's zeros are
            assert not bool(bad.any()), (f"{case.id}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                                         f"{[int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]}")
        if out32 is not None:
            assert _bands_intact(buf32, out32)
            assert torch.equal(_bits(out32), _bits(torch.from_numpy(d.want.astype(np.float32)).to(dev))), f"{case.id}: fp32 output"
    # a second call gives the same bits
    out.view(torch.int16 if case.y16 else torch.int32).fill_(-1)    # every byte 0xFF again
    _launch(case, t, out, out32=out32)
    assert torch.equal(_bits(out), _bits(first)), f"{case.id}: a second call differs"
    # image i of the batch equals image i alone (which may well take another route: the result may not depend on it)
    if not case.rows:
        for i in range(case.b) if case.b <= 3 else (0, case.b - 1):
            b1, o1 = _poisoned(_out_shape(case, 1), ydt, dev)
            _launch(case, _image(case, t, i), o1, b=1)
            whole = first[:, i:i + 1] if case.out_mode == 2 else first[i:i + 1]
            assert torch.equal(_bits(o1), _bits(whole)), f"{case.id}: image {i} alone differs from image {i} of the batch"
            assert _bands_intact(b1, o1)


_ID = lambda c: c.id


@pytest.mark.parametrize("case", FP32_CASES, ids=_ID)
def test_fp32_routes_are_exact(dev, case):
    """conv_bn_act / deconv2x2: every route of the fp32 dispatcher (tests/test_conv_exact_host.py holds the table)."""
    _run_exact(case, dev)


@pytest.mark.parametrize("case", C.f16mfma_cases(), ids=_ID)
def test_f16mfma_routes_are_exact(dev, case):
    """products = 1: fp16 operands (the integers are fp16 values), fp32 accumulation. products = 3: the operand that needs 13
    significand bits is split into hi + lo exactly and the other has no lo part, so the dropped lo x lo term is zero."""
    _run_exact(case, dev)


@pytest.mark.parametrize("case", C.f16io_cases(), ids=_ID)
def test_f16io_routes_are_exact(dev, case):
    """fp16 outputs are the exact value rounded once: numpy's float64 -> float16 (round to nearest even)."""
    _run_exact(case, dev)


@pytest.mark.parametrize("case", C.f16p_cases(), ids=_ID)
def test_f16_pipelined_is_exact_on_every_tile(dev, case):
    _run_exact(case, dev)


def test_fp32_cases_reach_every_route_on_this_device():
    """The routes are recomputed with this device's CU count: the reached set is again the whole reachable set."""
    assert coverage_problems(FP32_CASES, CUS) == []


def test_refused_combinations_raise(dev):
    """The io16 forms conv_f16.hip does not instantiate are errors, not results."""
    from maskrcnn_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    h = torch.float16
    w32, w24, w33 = z(64, 1, 1, 32, dt=h), z(64, 1, 1, 24, dt=h), z(33, 1, 1, 32, dt=h)
    call = ops.conv_bn_act_f16mfma
    with pytest.raises(RuntimeError, match="supports no residual / sigmoid / scatter"):      # fp32 -> fp16 + residual
        call(z(1, 4, 4, 32), w32, None, None, None, residual=z(1, 4, 4, 64, dt=h), products=1, out_f16=True)
    with pytest.raises(RuntimeError, match="supports no residual / sigmoid / scatter"):      # fp32 -> fp16 + sigmoid
        call(z(1, 4, 4, 32), w32, None, None, None, relu=2, products=1, out_f16=True)
    with pytest.raises(RuntimeError, match="no sigmoid"):                                    # fp16 -> fp16 + sigmoid
        call(z(1, 4, 4, 32, dt=h), w32, None, None, None, relu=2, products=1, out_f16=True)
    with pytest.raises(RuntimeError, match="no residual / scatter"):                         # fp16 -> fp32 + residual
        call(z(1, 4, 4, 32, dt=h), w32, None, None, None, residual=z(1, 4, 4, 64), products=1)
    with pytest.raises(RuntimeError, match="fp16 input needs Cin"):                          # fp16 input with generic K
        call(z(1, 4, 4, 24, dt=h), w24, None, None, None, products=1, out_f16=True)
    with pytest.raises(RuntimeError, match="even Cout"):                                     # fp16 output with an odd Cout
        call(z(1, 4, 4, 32), w33, None, None, None, products=1, out_f16=True)
    with pytest.raises(RuntimeError, match="plain-fp16 mode"):                               # fp16 activations with the x 3 split
        call(z(1, 4, 4, 32, dt=h), w32, w32, None, None, products=3)
    with pytest.raises(RuntimeError, match="even channel count"):                            # fp16 scatter with 7 channels
        ops.deconv2x2(z(1, 4, 4, 32, dt=h), (z(28, 1, 1, 32, dt=h), None), z(28), 0, 1)
    with pytest.raises(RuntimeError, match="float16"):                                       # the pipelined kernel reads fp16 only
        ops.conv_f16_pipelined(z(1, 4, 4, 64), z(64, 1, 1, 64, dt=h), None, None)


def test_fp32_to_fp16_input_conversion_rounds_to_nearest_even(dev):
    """The fp32 -> fp16 input path (products = 1, fp32 x, identity 1x1 weight, 64 channels): x on fp16 rounding ties, one fp32 ulp
    either side of them, in fp16's subnormal range and just below 65504 — the output is x.astype(float16) under numpy's round to
    nearest even, both as the fp16 output and widened in the fp32 output. conv_f16_pipelined takes fp16 input only
    (test_refused_combinations_raise), so it has no such path."""
    from maskrcnn_amd import ops
    rng = np.random.Generator(np.random.PCG64(16))
    bits = np.concatenate([rng.integers(0, 0x7BFF, 5000), rng.integers(0, 0x0400, 400), np.arange(0x7BF0, 0x7BFF)]).astype(np.uint16)
    lo = bits.view(np.float16).astype(np.float32)
    hi = (bits + 1).astype(np.uint16).view(np.float16).astype(np.float32)
    mid = (lo + hi) / 2                                      # exact in fp32: the tie between two neighbouring fp16 values
    pos = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(0)),
                          np.float32([65503.0, 65504.0, np.nextafter(np.float32(65520), np.float32(0)), 65488.0, 2.0 ** -25, 2.0 ** -24])])
    vals = np.concatenate([pos, -pos]).astype(np.float32)
    n = 64 * (vals.size // 64 // 4 * 4)
    x = rng.permutation(vals)[:n].reshape(1, 4, n // 256, 64)
    assert np.isfinite(x.astype(np.float16)).all()
    want = x.astype(np.float16) + np.float16(0)              # a sum that starts from +0 has no -0
    assert (want.astype(np.float32) != x).mean() > 0.9       # nearly every value is rounded
    assert (np.abs(want) < 2.0 ** -14).sum() > 100           # fp16 subnormals
    eye = torch.eye(64, dtype=torch.float16).view(64, 1, 1, 64).contiguous().to(dev)
    xd = torch.from_numpy(x).to(dev)
    got16 = ops.conv_bn_act_f16mfma(xd, eye, None, None, None, products=1, out_f16=True)
    got32 = ops.conv_bn_act_f16mfma(xd, eye, None, None, None, products=1)
    assert torch.equal(_bits(got16), _bits(torch.from_numpy(want).to(dev)))
    assert torch.equal(_bits(got32), _bits(torch.from_numpy(want.astype(np.float32)).to(dev)))
