"""GPU tests (-m gpu) of the conv backward: ops.conv_bn_act_backward (csrc/conv_backward.hip) and the differentiable front end
maskrcnn_amd.layers.

Exact data (conv_backward_cases): dx, dw, dshift, dresidual, g and z equal the float64 autograd result bit for bit, whatever the
chunking of the weight gradient and the route of the data gradient; tests/test_conv_backward_host.py asserts, without a GPU, the
conditions that make this a theorem. Rounded data: g and z against the rule restated in torch fp32, dw / dx / dshift against a
float64 evaluation from the op's own z within the forward error bound of a recursive fp32 sum of that length. The shapes are the
smallest at which each mechanism can go wrong. The file runs once more in a child pytest on the schedule-fuzz library."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_backward_cases as cb

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_LIB = os.path.join(ROOT, "maskrcnn_amd", "csrc", "build", "variants", "sync_fuzz", "libmaskrcnn_hip.so")
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from maskrcnn_amd import ops as o
    return o


def dev(t, dtype=F32):
    return None if t is None else t.to(dtype).contiguous().to(DEV)


def assert_same_bits(got, want64, what):
    """got (fp32, GPU) against a float64 expectation that fp32 holds exactly; -0 and +0 are the same number here."""
    assert got is not None, what
    got, want = got.detach().cpu(), want64.to(F32)
    assert torch.equal(want.to(F64), want64.to(F64)), f"{what}: the expectation is not an fp32 number"
    assert got.shape == want.shape and got.dtype == F32, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    same = (got + 0.0).view(torch.int32) == (want + 0.0).view(torch.int32)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ in their bits"


def gpu_inputs(c, d):
    """The case's operands on the GPU as the op takes them: scatter cases' dy and y scattered to [B,2H,2W,C]; every row the row
    groups switch off filled with NaN in x, y and grad_out."""
    x, dy, y = d.x.clone(), d.dy.clone(), d.y.clone()
    counts = None
    if c.counts:
        off = ~d.valid.reshape(-1)
        for t in (x, dy, y):
            t.reshape(c.m, -1)[off] = float("nan")
        counts = torch.tensor(c.counts, dtype=torch.int32, device=DEV)
    if c.scatter:
        dy, y = cb.scatter_nhwc(dy), cb.scatter_nhwc(y)
    return dev(x), dev(d.w), dev(dy), dev(y), dev(d.scale), counts


def run(ops, c, d, needs=None, **kw):
    x, w, dy, y, scale, counts = gpu_inputs(c, d)
    needs = (True, True, True, c.res_div != 0) if needs is None else needs
    r = ops.conv_bn_act_backward(dy, x, w, y, scale, c.pad, c.act, c.res_div, c.scatter, counts, c.rpg, needs=needs, **kw)
    torch.cuda.synchronize()
    return r, dy


# --------------------------------------------------------------------------------------------------------------- exact data
@pytest.mark.parametrize("name", [c.id for c in cb.cases()])
def test_exact_data_equal_float64_bit_for_bit(ops, name):
    c = cb.case(name)
    d = cb.build(c)
    r, dy = run(ops, c, d)
    assert_same_bits(r.z, d.z, f"{name}: z")
    assert_same_bits(r.dx, d.dx, f"{name}: dx")
    assert_same_bits(r.dw, d.dw, f"{name}: dw")
    assert_same_bits(r.dshift, d.dshift, f"{name}: dshift")
    if c.res_div:
        assert_same_bits(r.dresidual, d.dresidual, f"{name}: dresidual")
    if c.res_div == 1:
        assert_same_bits(r.dresidual, d.g, f"{name}: g")
    alias = c.act == 0 and not c.scale and not c.counts and not c.scatter and c.cout % 4 == 0
    assert (r.z.data_ptr() == dy.data_ptr()) == alias, f"{name}: z is dy itself exactly where the rule says so"
    if c.counts:
        off = ~d.valid.reshape(-1)
        for t, what in ((r.z, "z"), (r.dx, "dx")):
            assert not bool(t.cpu().reshape(c.m, -1)[off].view(torch.int32).any()), f"{name}: a switched-off {what} row is not +0"


def test_g_of_a_row_group_case_is_written_as_zero_where_switched_off(ops):
    """g itself is reachable as dresidual at res_div 1 only, which row groups exclude at the Python face: ask the library."""
    from maskrcnn_amd._lib import check, lib
    c = cb.case("rows_2x2")
    d = cb.build(c)
    x, w, dy, y, scale, counts = gpu_inputs(c, d)
    g = torch.full((c.b, *c.out_hw, c.cout), float("nan"), device=DEV)
    ws = torch.empty(16, dtype=torch.uint8, device=DEV)
    check(lib.mrcnn_conv_act_backward_f32(dy.data_ptr(), y.data_ptr(), c.b, *c.out_hw, c.cout, scale.data_ptr(), c.act, 0, 0,
                                          counts.data_ptr(), c.rpg, None, g.data_ptr(), None, None, ws.data_ptr(), 16,
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert_same_bits(g, d.g, "g")
    assert not bool(g.cpu().reshape(c.m, -1)[~d.valid.reshape(-1)].view(torch.int32).any())


# ------------------------------------------------------------------------------------------------------------- rounded data
@pytest.mark.parametrize("name", cb.ROUNDED)
def test_rounded_data_within_the_bound_of_a_recursive_fp32_sum(ops, name):
    c = cb.rounded_case(name)
    d = cb.build_rounded(c)
    relu = c.act == 1
    r = ops.conv_bn_act_backward(dev(d["dy"]), dev(d["x"]), dev(d["w"]), dev(d["y"]), dev(d["scale"]), c.pad, c.act,
                                 1 if relu else 0, needs=(True, True, True, relu))
    torch.cuda.synchronize()
    assert_same_bits(r.z, d["z"], f"{name}: z against the fp32 restatement")
    if relu:
        assert_same_bits(r.dresidual, d["g"], f"{name}: g against the fp32 restatement")
    kh, kw = c.k
    z64 = r.z.cpu().to(F64)[..., :c.cout]
    x64, w64 = d["x"].to(F64), d["w"].to(F64)
    dx64, dw64 = cb.conv_grads64(x64, w64, z64, c.pad)
    sum_zw, sum_zx = cb.conv_grads64(x64.abs(), w64.abs(), z64.abs(), c.pad)
    L = cb.chunk_of(c)
    dw_err, dw_bound = (r.dw.cpu().to(F64) - dw64).abs(), (L + 2) * U * sum_zx
    dx_err, dx_bound = (r.dx.cpu().to(F64) - dx64).abs(), (kh * kw * c.cout4 + 2) * U * sum_zw
    g64 = d["g"].to(F64).reshape(-1, c.cout)
    s = g64.sum(0)
    ds_err = (r.dshift.cpu().to(F64) - s).abs()
    ds_bound = U * s.abs() + g64.shape[0] * 2.0 ** -53 * g64.abs().sum(0)
    print(f"{name}: L {L}, chunks {-(-c.m // L)}; max |dw - dw64| / bound {float((dw_err / dw_bound).max()):.4f}, "
          f"max |dx - dx64| / bound {float((dx_err / dx_bound).max()):.4f}, max |dshift - s| / bound {float((ds_err / ds_bound).max()):.4f}")
    assert float(sum_zx.min()) > 0 and float(sum_zw.min()) > 0
    assert bool((dw_err <= dw_bound).all()), f"{name}: dw outside (L + 2) u sum|z||x| at {int((dw_err > dw_bound).sum())} elements"
    assert bool((dx_err <= dx_bound).all()), f"{name}: dx outside (KH KW Cout4 + 2) u sum|z||w| at {int((dx_err > dx_bound).sum())} elements"
    assert bool((ds_err <= ds_bound).all()), f"{name}: dshift outside u |s| + n 2^-53 sum|g|"


# --------------------------------------------------------------------------------------------------------------- properties
def rounded_call(ops, c, d, rows=slice(None), needs=(True, True, True, False)):
    r = ops.conv_bn_act_backward(dev(d["dy"][rows]), dev(d["x"][rows]), dev(d["w"]), dev(d["y"][rows]), dev(d["scale"]), c.pad, c.act,
                                 needs=needs)
    torch.cuda.synchronize()
    return r


def bits(t):
    return t.detach().cpu().view(torch.int32)


def test_two_calls_give_equal_bits(ops):
    c = cb.rounded_case("multi_chunk")
    d = cb.build_rounded(c)
    assert cb.chunks_of(c) >= 3
    a, b = rounded_call(ops, c, d), rounded_call(ops, c, d)
    for name in ("dx", "dw", "dshift", "z"):
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name


def test_dx_of_an_image_does_not_depend_on_the_rest_of_the_batch(ops):
    c = cb.rounded_case("3x3_ragged")
    d = cb.build_rounded(c)
    whole = rounded_call(ops, c, d)
    for i in range(c.b):
        alone = rounded_call(ops, c, d, rows=slice(i, i + 1))
        assert torch.equal(bits(alone.dx), bits(whole.dx[i:i + 1])), f"image {i}"
        assert torch.equal(bits(alone.z), bits(whole.z[i:i + 1])), f"image {i}: z"


def test_needs_switched_off_return_none_and_do_not_change_the_others(ops):
    c = cb.case("residual_1")
    d = cb.build(c)
    full, _ = run(ops, c, d)
    for k, name in enumerate(("dx", "dw", "dshift", "dresidual")):
        needs = [True] * 4
        needs[k] = False
        r, _ = run(ops, c, d, needs=tuple(needs))
        assert getattr(r, name) is None, name
        for other in ("dx", "dw", "dshift", "dresidual", "z"):
            if other != name:
                assert torch.equal(bits(getattr(r, other)), bits(getattr(full, other))), (name, other)
    only, _ = run(ops, c, d, needs=(False, False, True, False))
    assert only.dx is None and only.dw is None and only.dresidual is None and only.z is None
    assert torch.equal(bits(only.dshift), bits(full.dshift))
    nothing, _ = run(ops, c, d, needs=(False, False, False, False))
    assert all(v is None for v in nothing)


# ---------------------------------------------------------------------------------------------------------------- front end
def chain_data():
    rng = np.random.default_rng(7)
    t = lambda lim, *shape: torch.from_numpy(rng.integers(-lim, lim + 1, shape).astype(np.float64))
    b, h, w, cin, c1, c2, c3 = 2, 5, 3, 4, 8, 4, 6
    return dict(x=t(2, b, h, w, cin), w1=t(2, c1, 3, 3, cin), s1=torch.from_numpy(cb.channel_scale(c1)),
                t1=torch.from_numpy(cb.channel_shift(c1)), w4=t(2, 4 * c2, 1, 1, c1), bias=t(3, c2), w3=t(2, c3, 1, 1, c2),
                t3=torch.from_numpy(cb.channel_shift(c3)), weights=t(3, b, 2 * h, 2 * w, c3))


LEAVES = ("x", "w1", "t1", "w4", "bias", "w3", "t3")


def chain64(d, relu=True):
    """conv 3x3 SAME + BN affine + ReLU -> ConvTranspose2d(2, stride 2) + bias + ReLU -> conv 1x1 + shift, from F.conv2d and
    F.conv_transpose2d in float64; → the gradients of (y * weights).sum() in the leaves. relu=False with absolute values bounds
    every partial sum of the real graph."""
    p = {k: d[k].detach().clone().requires_grad_(True) for k in LEAVES}
    act = torch.relu if relu else (lambda v: v)
    y1 = act(cb.conv64(p["x"], p["w1"], (1, 1, 1, 1)) * d["s1"] + p["t1"])
    c2 = p["bias"].numel()
    wt = p["w4"].reshape(2, 2, c2, -1).permute(3, 2, 0, 1)                       # [Cin][C][dy][dx]
    y2 = act(F.conv_transpose2d(y1.permute(0, 3, 1, 2), wt, p["bias"], stride=2).permute(0, 2, 3, 1))
    y3 = cb.conv64(y2, p["w3"], (0, 0, 0, 0)) + p["t3"]
    (y3 * d["weights"]).sum().backward()
    return {k: v.grad for k, v in p.items()}, (y1.detach(), y2.detach(), y3.detach())


def test_a_chain_of_layers_gives_the_float64_graphs_gradients_bit_for_bit(ops):
    from maskrcnn_amd import layers
    d = chain_data()
    want, outs = chain64(d)
    bound, bound_outs = chain64({k: v.abs() for k, v in d.items()}, relu=False)
    worst = max(float(v.max()) for v in list(bound.values()) + list(bound_outs))
    assert worst * 2 < 2 ** 24, worst                                            # every partial sum an exact multiple of 1/2
    assert all(bool(v.any()) for v in want.values()) and 0.2 < float((outs[0] == 0).double().mean()) < 0.8
    p = {k: dev(d[k]).requires_grad_(True) for k in LEAVES}
    s1 = dev(d["s1"]).requires_grad_(True)
    y1 = layers.conv_bn_act(p["x"], p["w1"], s1, p["t1"], pad=(1, 1, 1, 1), act=1)
    y2 = layers.deconv2x2(y1, p["w4"], p["bias"].repeat(4), act=1)
    y3 = layers.conv_bn_act(y2, p["w3"], None, p["t3"])
    assert y3.grad_fn is not None
    assert_same_bits(y3, outs[2].detach(), "the chain's output")
    (y3 * dev(d["weights"])).sum().backward()
    torch.cuda.synchronize()
    for k in LEAVES:
        assert_same_bits(p[k].grad, want[k], f"gradient of {k}")
    assert s1.grad is None, "scale is frozen: no gradient"
    # the inference call is unchanged: nothing saved, no grad_fn
    plain = ops.conv_bn_act(p["x"], p["w1"], s1, p["t1"], pad=(1, 1, 1, 1), relu=1)
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, y1.detach())
    assert ops.deconv2x2(y1, p["w4"], p["bias"].detach().repeat(4), 1).grad_fn is None


def test_layers_residual_and_row_groups_reach_their_gradients(ops):
    from maskrcnn_amd import layers
    c = cb.case("residual_2")
    d = cb.build(c)
    x, w, shift, res = [dev(t).requires_grad_(True) for t in (d.x, d.w, d.shift, d.residual)]
    y = layers.conv_bn_act(x, w, dev(d.scale), shift, pad=c.pad, act=c.act, residual=res, res_div=2)
    assert_same_bits(y, d.y, "forward")
    y.backward(dev(d.dy))
    for got, want, what in ((x.grad, d.dx, "dx"), (w.grad, d.dw, "dw"), (shift.grad, d.dshift, "dshift"), (res.grad, d.dresidual, "dres")):
        assert_same_bits(got, want, what)
    c = cb.case("rows")
    d = cb.build(c)
    xg, wg, dy, _, scale, counts = gpu_inputs(c, d)
    xg, wg = xg.requires_grad_(True), wg.requires_grad_(True)
    y = layers.conv_bn_act(xg, wg, scale, dev(d.shift), act=1, row_counts=counts, rows_per_group=c.rpg)
    y.backward(dy)                                    # NaN in every switched-off row of x and of the incoming gradient
    assert_same_bits(xg.grad, d.dx, "rows: dx")
    assert_same_bits(wg.grad, d.dw, "rows: dw")


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_bad_shapes_and_dtypes_are_refused_with_the_house_message(ops):
    op = ops.conv_bn_act_backward
    x, w, g = torch.zeros(1, 4, 4, 8, device=DEV), torch.zeros(6, 3, 3, 8, device=DEV), torch.zeros(1, 4, 4, 6, device=DEV)
    same = dict(pad=(1, 1, 1, 1))
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: grad_out must be float32 \[1,4,4,6\], got float32 \[1, 4, 3, 6\]"):
        op(g[:, :, :3], x, w, None, **same)
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: w must be float32 \[Cout>=1,KH>=1,KW>=1,8\], got float32 \[6, 3, 3, 4\]"):
        op(g, x, w[..., :4], None, **same)
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: x must be float32 \[B>=1,H>=1,W>=1,Cin>=4\], got float64"):
        op(g, x.double(), w, None, **same)
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: x must be float32 \[B,H,W,Cin\] with Cin a multiple of 4"):
        op(g, x[..., :6], w[..., :6], None, **same)
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: pad must be \(top, left, bottom, right\) in 0 .. kernel size - 1 = \(2, 2\), got \(3, 1, 1, 1\)"):
        op(g, x, w, None, pad=(3, 1, 1, 1))
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: y must be float32 \[1,4,4,6\], got None"):
        op(g, x, w, None, act=1, **same)
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: scale must be float32 \[6\] or None, got float32 \[5\]"):
        op(g, x, w, None, torch.ones(5, device=DEV), **same)
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: row_counts must be int32 \[4\], got int64"):
        op(g, x, w, None, row_counts=torch.zeros(4, dtype=torch.int64, device=DEV), rows_per_group=4, **same)
    with pytest.raises(RuntimeError, match="conv_bn_act_backward: row_counts must be None with a residual or the scatter, or with rows_per_group"):
        op(g, x, w, None, row_counts=torch.zeros(4, dtype=torch.int32, device=DEV), rows_per_group=5, **same)
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: w must be float32 \[4\*C,1,1,8\] without padding for the scatter"):
        op(g, x, w, None, scatter=True, **same)
    with pytest.raises(RuntimeError, match=r"conv_bn_act_backward: res_div must be 1 for an odd output size \(3 x 3\)"):
        op(g[:, :3, :3], x[:, :3, :3], w, None, res_div=2, needs=(True, True, True, True), **same)


# --------------------------------------------------------------------------------------------------------- schedule fuzzing
# The child's time limit: four times the wall time measured on the fuzzed library, rounded up to 30 s: 5.2 s (25 tests; 3 s of it
# inside pytest, the rest start-up), so 20.9 s -> 30 s.
FUZZ_TIMEOUT = 30


@pytest.mark.skipif(os.environ.get("MRCNN_SYNC_FUZZ_CHILD") == "1", reason="this IS the fuzzed child run")
def test_this_file_passes_under_schedule_fuzzing():
    """conv_wgrad_f32 hands a k tile's operands and the pixel table of the next one from wave to wave through LDS with one barrier
    per k tile; on that build every wave sleeps a random time behind each barrier, and a hand-off that the barrier does not order
    fails its bit comparison there."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_conv_backward.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=FUZZ_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
