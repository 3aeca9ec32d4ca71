"""GPU tests of the clipped SGD (csrc/optim.hip through maskrcnn_amd.optim.ClippedSGD and ops.grad_clip_coef / ops.sgd_apply) against
the reference's composition in float64 on the CPU; the table, the reference and the bars are tests/optim_cases.py's. The last test
runs this file once more on the schedule-fuzz build."""
import math
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_LIB = os.path.join(ROOT, "maskrcnn_amd", "csrc", "build", "variants", "sync_fuzz", "libmaskrcnn_hip.so")
DEV = torch.device("cuda:0")
_cases, _wants = {}, {}


def _case(kw):
    from maskrcnn_amd import optim
    key = tuple(sorted(kw.items()))
    if key not in _cases:
        _cases[key] = oc.Case(optim.TILE, **kw)
    return _cases[key]


def _want(name, kw, hyper, mode):
    """One reference per configuration, shared and left unchanged."""
    if name not in _wants:
        _wants[name] = oc.reference(_case(kw), hyper["lr"], hyper["momentum"], hyper["wd"], hyper["max_norm"], mode)
    return _wants[name]


def _state_bits(opt, ps):
    return [(oc.bits(q), oc.bits(opt.state[q]["momentum_buffer"]), None if q.grad is None else oc.bits(q.grad)) for q in ps]


# ------------------------------------------------------------------------------------------------ the table against the reference
@pytest.mark.parametrize("name", list(oc.CONFIGS))
def test_table_against_the_float64_reference(name):
    from maskrcnn_amd import optim
    kw, hyper, mode = oc.CONFIGS[name]
    case, want = _case(kw), _want(name, kw, hyper, mode)
    opt, ps, norm = oc.run_case(optim, case, hyper, mode, DEV)
    worst, rel = oc.compare(case, opt, ps, norm, want, optim.TILE)
    print(f"{name}: worst {worst:.3f} ulp, norm rel {rel:.2e} (bound {oc.norm_bound(optim.TILE, oc.tiles_of(case, optim.TILE)):.2e})")
    if mode == "step_zero":
        assert all(not oc.bits(q.grad).any() for q in ps if q.grad is not None)      # +0, not -0
    if mode == "clip":
        assert all(torch.equal(oc.bits(q), oc.bits(p)) for q, p in zip(ps, case.p))
        assert all(torch.equal(oc.bits(opt.state[q]["momentum_buffer"]), oc.bits(b)) for q, b in zip(ps, case.b))
    if name == "no max_norm":
        assert norm is None


def test_sum_of_squares_has_the_stated_order():
    """S through the binding, bit for bit what the numpy restatement of the kernels' order gives, with the tiles of the tensor
    without a gradient in their place; the aligned and the scalar path add the same bits."""
    from maskrcnn_amd import ops, optim
    case = _case({})
    ps = case.params(DEV)
    bufs = [torch.zeros_like(p) for p in ps]
    host = optim.build_table([(p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr(), b.data_ptr(), p.numel(), 0.0) for p, b in zip(ps, bufs)])
    assert not host.aligned[case.view] and host.aligned[case.twin]
    table, tile_off = torch.from_numpy(host.table).to(DEV), torch.from_numpy(host.tile_off).to(DEV)
    info, status = ops.grad_clip_coef(table, tile_off, 5.0, tiles=host.tiles)
    info2, _ = ops.grad_clip_coef(table, tile_off, 5.0)            # tiles read back from tile_off
    s = optim.sumsq_fixed_order([(None if g is None else g.numpy(), p.numel()) for g, p in zip(case.g, case.p)])
    assert info.tolist()[0] == s and torch.equal(info.view(torch.int64), info2.view(torch.int64)) and status.tolist() == [0]
    assert info.tolist()[1] == math.sqrt(s) and info.tolist()[2] == min(1.0, 5.0 / (math.sqrt(s) + 1e-6))


def test_exact_case_equals_float64_and_torch_fp32_bit_for_bit():
    from maskrcnn_amd import optim
    kw, hyper, mode = oc.EXACT
    case, want = _case(kw), _want("exact", kw, hyper, mode)
    opt, ps, norm = oc.run_case(optim, case, hyper, mode, DEV)
    qs = case.params("cpu")                                        # torch's own fp32 path on the same state
    torch.nn.utils.clip_grad_norm_(qs, hyper["max_norm"])
    ref = torch.optim.SGD(case.groups(qs, hyper["wd"]), lr=hyper["lr"], momentum=hyper["momentum"])
    for q, b in zip(qs, case.b):
        ref.state[q]["momentum_buffer"] = b.clone()
    ref.step()
    for i, (q, r) in enumerate(zip(ps, qs)):
        if case.g[i] is None:
            continue
        b = opt.state[q]["momentum_buffer"]
        assert torch.equal(oc.bits(q), oc.bits(want["p"][i].float())) and torch.equal(oc.bits(q), oc.bits(r)), i
        assert torch.equal(oc.bits(b), oc.bits(want["b"][i].float())) and torch.equal(oc.bits(b), oc.bits(ref.state[r]["momentum_buffer"])), i
        assert torch.equal(oc.bits(q.grad), oc.bits(case.g[i])), i
    assert float(norm) == want["norm"] and opt.status.tolist() == [0]


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_non_finite_gradient_sets_status_and_changes_nothing_but_the_zeroing(value):
    from maskrcnn_amd import optim
    base = _case({})
    for mode in ("clip", "step", "step_zero"):
        ps = base.params(DEV)
        big = max(range(len(ps)), key=lambda i: ps[i].numel())
        ps[big].grad[3 * optim.TILE + 2] = value                   # in the middle of the long tensor
        grads = [None if q.grad is None else q.grad.clone() for q in ps]
        opt = optim.ClippedSGD(base.groups(ps, 1e-4), lr=0.01, momentum=0.9, max_norm=5.0)
        base.load_buffers(opt, ps)
        norm = opt.clip_() if mode == "clip" else opt.step(zero_grad=mode == "step_zero")
        assert opt.status.tolist() == [1] and not math.isfinite(float(norm))
        for i, q in enumerate(ps):
            assert torch.equal(oc.bits(q), oc.bits(base.p[i])) and torch.equal(oc.bits(opt.state[q]["momentum_buffer"]), oc.bits(base.b[i])), (mode, i)
            if q.grad is not None:
                want = torch.zeros_like(grads[i]) if mode == "step_zero" else grads[i]
                assert torch.equal(oc.bits(q.grad), oc.bits(want)), (mode, i)


def test_two_calls_on_cloned_state_give_the_same_bits():
    from maskrcnn_amd import optim
    kw, hyper, _ = oc.CONFIGS["clipped step"]
    runs = []
    for _ in range(2):
        opt, ps, norm = oc.run_case(optim, _case(kw), hyper, "step", DEV)
        runs.append((_state_bits(opt, ps), oc.bits(norm.reshape(1))))
    for (a, b, c), (d, e, f) in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, d) and torch.equal(b, e) and (c is None and f is None or torch.equal(c, f))
    assert torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------ the front end
def _checked(opt, ps, decay, mode, hyper=oc.H):
    """One call of the code under test from whatever state it is in, against the reference fed with that state."""
    from maskrcnn_amd import optim
    snap = oc.Snapshot(opt, ps, decay)
    norm = opt.clip_() if mode == "clip" else opt.step(zero_grad=mode == "step_zero")
    want = oc.reference(snap, hyper["lr"], hyper["momentum"], hyper["wd"], hyper["max_norm"], mode)
    return oc.compare(snap, opt, ps, norm, want, optim.TILE)


def _toy(gen):
    from maskrcnn_amd import optim
    shapes = [(optim.TILE + 5,), (37, 3), (8,), (2, 3, 5)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=gen).to(DEV)) for s in shapes]
    decay = [True, True, False, False]
    opt = optim.ClippedSGD([{"params": ps[:2], "weight_decay": oc.H["wd"]}, {"params": ps[2:]}], lr=oc.H["lr"],
                           momentum=oc.H["momentum"], max_norm=oc.H["max_norm"])
    return ps, decay, opt


def _backward(ps, gen, scale=3.0):
    loss = sum(((q * torch.randn(q.shape, generator=gen).to(DEV)) ** 2).sum() + (q * scale).sum() for q in ps)
    loss.backward()


def test_accumulation_pattern_of_the_reference():
    """BATCH_SIZE = 2 (model.py:1632-1637): clip_() after the first backward, step(zero_grad=True) after the second, which has
    added its gradient to the clipped first one; three rounds, each call against the reference fed with the captured state."""
    gen = torch.Generator().manual_seed(5)
    ps, decay, opt = _toy(gen)
    for _ in range(3):
        _backward(ps, gen)
        _checked(opt, ps, decay, "clip")
        _backward(ps, gen)
        _checked(opt, ps, decay, "step_zero")
        assert all(not oc.bits(q.grad).any() for q in ps)


def test_replaced_and_dropped_gradients_rebuild_the_table():
    gen = torch.Generator().manual_seed(6)
    ps, decay, opt = _toy(gen)
    _backward(ps, gen)
    _checked(opt, ps, decay, "step")
    first = opt._device_table[0]
    _checked(opt, ps, decay, "step")
    assert opt._device_table[0] is first                           # nothing moved: the same table
    keep = [q.grad for q in ps]                                    # the old tensors stay alive: a stale table would write into them
    for q in ps:
        q.grad = torch.randn(q.shape, generator=gen).to(DEV)
    old = [g.clone() for g in keep]
    _checked(opt, ps, decay, "step")
    assert opt._device_table[0] is not first and all(torch.equal(a, b) for a, b in zip(keep, old))
    opt.zero_grad(set_to_none=True)
    assert all(q.grad is None for q in ps)
    before = _state_bits(opt, ps)
    opt.step()                                                     # every tensor skipped
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(before, _state_bits(opt, ps)))
    ps[1].requires_grad_(False)                                    # one tensor without a gradient beside fresh ones
    _backward([ps[0], ps[2], ps[3]], gen)
    _checked(opt, ps, decay, "step_zero")
    opt.state[ps[0]]["momentum_buffer"] = opt.state[ps[0]]["momentum_buffer"].clone()     # a replaced buffer
    _backward([ps[0], ps[2], ps[3]], gen)
    _checked(opt, ps, decay, "step")


def test_two_steps_through_conv_bn_act():
    """The gradients this project's autograd functions deliver are accepted as they arrive."""
    from maskrcnn_amd import layers, optim
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 6, 5, 8, generator=gen).to(DEV)
    w = torch.nn.Parameter((torch.randn(12, 3, 3, 8, generator=gen) * 0.2).to(DEV))
    shift = torch.nn.Parameter(torch.randn(12, generator=gen).to(DEV))
    opt = optim.ClippedSGD([{"params": [w], "weight_decay": oc.H["wd"]}, {"params": [shift]}], lr=oc.H["lr"], momentum=oc.H["momentum"],
                           max_norm=oc.H["max_norm"])
    for _ in range(2):
        y = layers.conv_bn_act(x, w, None, shift, pad=(1, 1, 1, 1), act=1)
        (y * y).sum().backward()
        _checked(opt, [w, shift], [True, False], "step_zero")


def test_bad_arguments_are_refused_before_anything_is_launched():
    from maskrcnn_amd import ops, optim
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=DEV)
    table, off, wd = i64(3, 4), i64(4), torch.zeros(3, dtype=torch.float64, device=DEV)
    info, status = torch.zeros(3, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    clip = lambda **kw: ops.grad_clip_coef(**{**dict(table=table, tile_off=off, max_norm=5.0, tiles=0), **kw})
    appl = lambda **kw: ops.sgd_apply(**{**dict(table=table, wd=wd, tile_off=off, info=info, status=status, lr=0.1, momentum=0.9, mode="step",
                                                tiles=0), **kw})
    nan, inf = float("nan"), float("inf")
    for call, kw, text in ((clip, dict(table=i64(65536, 4), tile_off=i64(65537)), "grad_clip_coef: table must be"),
                           (clip, dict(table=i64(3, 3)), "grad_clip_coef: table must be int64"),
                           (clip, dict(tile_off=i64(3)), "grad_clip_coef: tile_off must be int64"),
                           (clip, dict(tiles=2 ** 24 + 1), "grad_clip_coef: tiles must be"), (clip, dict(tiles=-1), "grad_clip_coef: tiles must be"),
                           (clip, dict(max_norm=0.0), "grad_clip_coef: max_norm must be"), (clip, dict(max_norm=nan), "grad_clip_coef: max_norm must be"),
                           (clip, dict(max_norm=None), "grad_clip_coef: max_norm must be"),
                           (appl, dict(table=i64(65536, 4), tile_off=i64(65537), wd=torch.zeros(65536, dtype=torch.float64, device=DEV)),
                            "sgd_apply: table must be"),
                           (appl, dict(wd=wd.float()), "sgd_apply: wd must be float64"), (appl, dict(tiles=2 ** 24 + 1), "sgd_apply: tiles must be"),
                           (appl, dict(lr=nan), "sgd_apply: lr must be"), (appl, dict(lr=inf), "sgd_apply: lr must be"),
                           (appl, dict(momentum=1.0), "sgd_apply: momentum must be"), (appl, dict(momentum=-0.5), "sgd_apply: momentum must be"),
                           (appl, dict(momentum=nan), "sgd_apply: momentum must be"), (appl, dict(mode=3), "sgd_apply: mode must be"),
                           (appl, dict(mode="zero"), "sgd_apply: mode must be"), (appl, dict(status=None), "sgd_apply: status must be"),
                           (appl, dict(info=info.float()), "sgd_apply: info must be float64")):
        with pytest.raises(RuntimeError, match=text):
            call(**kw)
    # what only the table's builder sees
    for entries, text in (([(16, 16, 16, 2 ** 31, 0.0)], "sgd_table: numel"), ([(16, 16, 16, 4, inf)], "sgd_table: wd"),
                          ([(16, 16, 16, 2 ** 31 - 1, 0.0)] * 33, "sgd_table: tiles")):
        with pytest.raises(RuntimeError, match=text):
            optim.build_table(entries)
    # and the calls that are fine: an empty table's worth of tiles launches the finishing workgroup alone
    got, st = clip()
    assert got.tolist() == [0.0, 0.0, 1.0] and st.tolist() == [0]
    appl()


# --------------------------------------------------------------------------------------------------------- schedule fuzzing
# The child's time limit: four times the wall time measured on the fuzzed library, rounded up to 30 s: 8.5 s (18 tests; 5.7 s of it
# inside pytest — the float64 references on the CPU, math.fsum over a million squares each, are most of that —, the rest start-up),
# so 34.2 s -> 60 s.
FUZZ_TIMEOUT = 60


@pytest.mark.skipif(os.environ.get("MRCNN_SYNC_FUZZ_CHILD") == "1", reason="this IS the fuzzed child run")
def test_this_file_passes_under_schedule_fuzzing():
    """optim_sumsq and optim_finish reduce through block_sum's two barriers (csrc/workgroup.hpp); on that build every wave sleeps a
    random time behind each barrier, and a sum that reads the LDS partials before they are all there fails its bit comparison."""
    assert os.path.exists(FUZZ_LIB), f"{FUZZ_LIB} is missing: run __graft_entry__.build()"
    env = dict(os.environ, MRCNN_LIB=FUZZ_LIB, MRCNN_SYNC_FUZZ_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_optim.py", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=FUZZ_TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
