"""Host tests of the clipped SGD (maskrcnn_amd/optim.py, csrc/optim.hip): the numpy path of ClippedSGD on CPU parameters against
the reference's composition in float64 (tests/optim_cases.py), the table builder, the refused configurations, the state_dict
round trip with torch.optim.SGD, and the boundary (ABI, the unregistered bindings, the build flags). No GPU."""
import copy
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_cases as oc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.mark.parametrize("name", list(oc.CONFIGS))
def test_numpy_path_against_the_float64_reference(name):
    from maskrcnn_amd import optim
    kw, hyper, mode = oc.CONFIGS[name]
    case = oc.Case(optim.TILE, **kw)
    want = oc.reference(case, hyper["lr"], hyper["momentum"], hyper["wd"], hyper["max_norm"], mode)
    opt, ps, norm = oc.run_case(optim, case, hyper, mode, CPU)
    worst, rel = oc.compare(case, opt, ps, norm, want, optim.TILE)
    print(f"{name}: worst {worst:.3f} ulp, norm rel {rel:.2e}, clipped {want['clipped']}")
    assert want["clipped"] == name.startswith(("clipped", "momentum", "lr", "large"))
    if mode == "step_zero":
        assert all(not oc.bits(q.grad).any() for q in ps if q.grad is not None)      # +0, not -0
    if mode == "clip":
        assert all(torch.equal(q.detach(), p) for q, p in zip(ps, case.p))


def test_exact_case_equals_float64_and_torch_fp32_bit_for_bit():
    from maskrcnn_amd import optim
    kw, hyper, mode = oc.EXACT
    case = oc.Case(optim.TILE, **kw)
    want = oc.reference(case, hyper["lr"], hyper["momentum"], hyper["wd"], hyper["max_norm"], mode)
    opt, ps, norm = oc.run_case(optim, case, hyper, mode, CPU)
    # torch's own fp32 path on the same state
    qs = case.params(CPU)
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
    assert float(norm) == want["norm"]      # integer squares: every partial sum is exact


def test_non_finite_gradient_sets_status_and_changes_nothing_but_the_zeroing():
    from maskrcnn_amd import optim
    for value in (float("nan"), float("inf")):
        for mode in ("clip", "step", "step_zero"):
            case = oc.Case(optim.TILE)
            case.g[7][5] = value
            opt, ps, norm = _run_unchecked(optim, case, mode)
            assert opt.status.tolist() == [1] and not np.isfinite(float(norm))
            for i, q in enumerate(ps):
                assert torch.equal(oc.bits(q), oc.bits(case.p[i])) and torch.equal(oc.bits(opt.state[q]["momentum_buffer"]), oc.bits(case.b[i]))
                if q.grad is not None:
                    want = torch.zeros_like(case.g[i]) if mode == "step_zero" else case.g[i]
                    assert torch.equal(oc.bits(q.grad), oc.bits(want)), (mode, i)


def _run_unchecked(optim, case, mode, hyper=oc.H):
    return oc.run_case(optim, case, hyper, mode, CPU)


def test_sumsq_restates_the_kernels_order():
    """sumsq_fixed_order: two calls agree, the sum lies within the summation depth's bound of the exact one (math.fsum), integer
    squares come out exactly, and tensors without a gradient or without elements add nothing."""
    import math
    from maskrcnn_amd import optim
    rng = np.random.default_rng(0)
    g = rng.standard_normal(3 * optim.TILE + 17).astype(np.float32)
    a = optim.sumsq_fixed_order([(g, g.size), (None, 9), (g[:5], 5)])
    assert a == optim.sumsq_fixed_order([(g, g.size), (None, 9), (g[:5], 5)])
    exact = math.fsum(float(v) * float(v) for v in np.concatenate([g, g[:5]]).astype(np.float64))
    assert abs(a - exact) <= 2 * oc.norm_bound(optim.TILE, 5) * exact
    ints = rng.integers(-9, 10, 2 * optim.TILE + 3).astype(np.float32)
    assert optim.sumsq_fixed_order([(ints, ints.size)]) == float((ints.astype(np.float64) ** 2).sum())
    assert optim.sumsq_fixed_order([(None, 4), (np.zeros(0, np.float32), 0)]) == 0.0


def test_table_builder():
    from maskrcnn_amd import optim
    t0 = optim.TILE
    assert t0 == int(__import__("maskrcnn_amd")._lib.lib.mrcnn_optim_tile()) and t0 % 1024 == 0
    entries = [(4096, 8192, 12288, 1, 0.5), (4096, 0, 12288, t0 + 1, 0.0), (4096, 8192, 12288, 0, 0.0), (4100, 8192, 12288, t0, 1e-4),
               (4096, 8192 + 8, 12288, 2 * t0, 0.0), (4096, 8192, 12288 + 4, 3, 0.0)]
    tab = optim.build_table(entries)
    assert tab.table.dtype == np.int64 and tab.table.shape == (6, 4) and tab.table.tolist() == [list(e[:4]) for e in entries]
    assert tab.wd.dtype == np.float64 and tab.wd.tolist() == [e[4] for e in entries]
    assert tab.tile_off.dtype == np.int64 and tab.tile_off.tolist() == [0, 1, 3, 3, 4, 6, 7] and tab.tiles == 7   # a null gradient keeps its tiles
    assert tab.aligned.tolist() == [True, True, True, False, False, False]
    for bad, text in (([], "number of tensors"), ([entries[0]] * 65536, "number of tensors"), ([(16, 16, 16, 2 ** 31, 0.0)], "numel"),
                      ([(16, 16, 16, -1, 0.0)], "numel"), ([(16, 16, 16, 4, float("nan"))], "wd"), ([(16, 16, 16, 4, float("inf"))], "wd"),
                      ([(16, 16, 16, 2 ** 31 - 1, 0.0)] * 33, "tiles")):
        with pytest.raises(RuntimeError, match="sgd_table: .*" + text):
            optim.build_table(bad)
    assert optim.build_table([(16, 16, 16, 2 ** 31 - 1, 0.0)] * 32).tiles == 2 ** 24


def test_refused_configurations():
    from maskrcnn_amd.optim import ClippedSGD
    P = lambda *shape, **kw: torch.nn.Parameter(torch.zeros(*shape, **kw))

    def refused(text, make, call=True):
        with pytest.raises(ValueError, match=text):
            opt = make()
            if call:
                opt.step()

    refused("differ in weight_decay only", lambda: ClippedSGD([{"params": [P(3)], "lr": 0.1}, {"params": [P(2)]}], lr=0.2))
    refused("differ in weight_decay only", lambda: ClippedSGD([{"params": [P(3)], "momentum": 0.5}, {"params": [P(2)]}], lr=0.2))
    refused("differ in weight_decay only", lambda: ClippedSGD([{"params": [P(3)], "max_norm": 1.0}, {"params": [P(2)]}], lr=0.2))
    refused("nesterov", lambda: ClippedSGD([{"params": [P(3)], "nesterov": True}], lr=0.2))
    refused("dampening", lambda: ClippedSGD([{"params": [P(3)], "dampening": 0.1}], lr=0.2))
    refused("dense contiguous float32", lambda: ClippedSGD([P(3, dtype=torch.float64)], lr=0.1))
    refused("dense contiguous float32", lambda: ClippedSGD([P(3, dtype=torch.float16)], lr=0.1))
    refused("dense contiguous float32", lambda: ClippedSGD([torch.nn.Parameter(torch.zeros(4, 4).t()[1:])], lr=0.1))
    refused("momentum must be in", lambda: ClippedSGD([P(3)], lr=0.1, momentum=1.0))
    refused("max_norm must be above 0", lambda: ClippedSGD([P(3)], lr=0.1, max_norm=0.0))
    refused("lr must be finite", lambda: ClippedSGD([P(3)], lr=float("inf")))
    refused("clip_\\(\\) needs a max_norm", lambda: ClippedSGD([P(3)], lr=0.1, max_norm=None).clip_(), call=False)
    if torch.cuda.is_available():
        refused("more than one device", lambda: ClippedSGD([P(3), P(3, device="cuda")], lr=0.1))
    else:
        refused("more than one device", lambda: ClippedSGD([P(3), P(3, device="meta")], lr=0.1))
    # a change after construction is caught at call time
    opt = ClippedSGD([{"params": [P(3)]}, {"params": [P(2)]}], lr=0.1)
    opt.param_groups[1]["lr"] = 0.01
    with pytest.raises(ValueError, match="differ in weight_decay only"):
        opt.step()
    # gradients: sparse, another dtype, another shape, not contiguous
    for grad in (torch.zeros(4, 4).to_sparse(), torch.zeros(4, 4, dtype=torch.float64), torch.zeros(16), torch.zeros(4, 8)[:, ::2]):
        p = P(4, 4)
        opt = ClippedSGD([p], lr=0.1)
        try:
            p.grad = grad
        except (RuntimeError, TypeError):      # torch itself refuses some of these assignments
            continue
        with pytest.raises(ValueError, match="a gradient must be a contiguous float32 tensor"):
            opt.step()


def test_lr_scheduler_and_group_lr_are_read_at_call_time():
    from maskrcnn_amd.optim import ClippedSGD
    p = torch.nn.Parameter(torch.ones(4))
    opt = ClippedSGD([p], lr=0.5, momentum=0.0, max_norm=None)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    p.grad = torch.ones(4)
    assert opt.step() is None and opt.status.tolist() == [0]
    sched.step()
    opt.step()
    assert p.tolist() == [0.25] * 4 and opt.param_groups[0]["lr"] == 0.25
    opt.zero_grad()
    assert p.grad is not None and not p.grad.any()
    opt.zero_grad(set_to_none=True)
    assert p.grad is None
    opt.step()                                   # a None gradient: the tensor is skipped
    assert p.tolist() == [0.25] * 4


def test_state_dict_round_trip_with_torch_sgd():
    from maskrcnn_amd.optim import ClippedSGD
    gen = torch.Generator().manual_seed(3)
    make = lambda: [torch.nn.Parameter(torch.randn(5, generator=torch.Generator().manual_seed(i))) for i in range(3)]
    grads = [torch.randn(5, generator=gen) * 0.1 for _ in range(3)]

    def groups(ps):
        return [{"params": ps[:2], "weight_decay": 1e-2}, {"params": ps[2:]}]

    def stepped(opt, ps):
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()

    # ours -> torch: buffers from construction (zeros) and after a step
    a, b = make(), make()
    ours, theirs = ClippedSGD(groups(a), lr=0.1, momentum=0.9, max_norm=1e9), torch.optim.SGD(groups(b), lr=0.1, momentum=0.9)
    assert all(not ours.state[p]["momentum_buffer"].any() for p in a)
    stepped(ours, a)
    stepped(theirs, b)
    for p, q in zip(a, b):
        assert torch.allclose(p, q, rtol=1e-6, atol=1e-7) and torch.allclose(ours.state[p]["momentum_buffer"], theirs.state[q]["momentum_buffer"], rtol=1e-6)
    c = make()
    fresh = torch.optim.SGD(groups(c), lr=0.5, momentum=0.1)
    fresh.load_state_dict(copy.deepcopy(ours.state_dict()))      # torch may keep the very tensors it is given
    assert fresh.param_groups[0]["lr"] == 0.1 and fresh.param_groups[0]["weight_decay"] == 1e-2 and fresh.param_groups[1]["weight_decay"] == 0
    for p, q in zip(a, c):
        assert torch.equal(fresh.state[q]["momentum_buffer"], ours.state[p]["momentum_buffer"])
        q.data.copy_(p.data)
    stepped(fresh, c)
    stepped(ours, a)
    for p, q in zip(a, c):
        assert torch.allclose(p, q, rtol=1e-6, atol=1e-7)
    # torch -> ours, with buffers, and from a torch state that has none (never stepped): zeros
    d = make()
    mine = ClippedSGD(groups(d), lr=0.5, momentum=0.1, max_norm=3.0)
    mine.load_state_dict(copy.deepcopy(theirs.state_dict()))
    assert mine.param_groups[0]["momentum"] == 0.9 and mine.param_groups[0]["max_norm"] == 3.0
    for p, q in zip(b, d):
        assert torch.equal(mine.state[q]["momentum_buffer"], theirs.state[p]["momentum_buffer"])
    e = make()
    mine = ClippedSGD(groups(e), lr=0.5, max_norm=None)
    mine.load_state_dict(torch.optim.SGD(groups(make()), lr=0.1, momentum=0.9).state_dict())
    assert all(mine.state[p]["momentum_buffer"].shape == p.shape and not mine.state[p]["momentum_buffer"].any() for p in e)
    stepped(mine, e)


def test_boundary_abi_bindings_and_build_flags():
    import maskrcnn_amd
    from maskrcnn_amd import _lib, ops, optim
    assert _lib.header_abi_version() >= 31 and int(_lib.lib.mrcnn_abi_version()) == _lib.header_abi_version()
    assert maskrcnn_amd.optim is optim and "optim" in maskrcnn_amd.__all__
    for name in ("grad_clip_coef", "sgd_apply"):
        assert callable(getattr(ops, name)) and name not in ops.__all__ and not hasattr(torch.ops.maskrcnn, name)
    spec = importlib.util.spec_from_file_location("_mrcnn_build_flags", os.path.join(ROOT, "maskrcnn_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "-ffp-contract=off" in build.SOURCES["optim.hip"]
    protos = _lib.header_prototypes()
    import ctypes
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert protos["mrcnn_optim_tile"] == (i32, [])
    assert protos["mrcnn_optim_clip_coef"] == (ctypes.c_int, [vp, vp, i32, i64, f64, vp, vp, vp, vp])
    assert protos["mrcnn_optim_sgd_apply"] == (ctypes.c_int, [vp, vp, vp, i32, i64, vp, vp, f64, f64, i32, vp])


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Dummy pointers, never touched: every refusal returns before a HIP call."""
    import ctypes
    from maskrcnn_amd import _lib
    lib = _lib.lib
    dp, N = ctypes.c_void_p(4096), None
    clip = lambda table=dp, off=dp, t=3, tiles=5, mx=5.0, ws=dp, info=dp, st=dp: lib.mrcnn_optim_clip_coef(table, off, t, tiles, mx, ws, info, st, N)
    appl = lambda table=dp, wd=dp, off=dp, t=3, tiles=5, lr=0.1, mom=0.9, mode=1: lib.mrcnn_optim_sgd_apply(table, wd, off, t, tiles, N, N, lr, mom, mode, N)
    nan, inf = float("nan"), float("inf")
    for call, kw, text in ((clip, dict(table=N), b"optim_clip_coef: null pointer"), (clip, dict(ws=N), b"optim_clip_coef: null pointer"),
                           (clip, dict(t=0), b"num_tensors=0"), (clip, dict(t=65536), b"num_tensors=65536"), (clip, dict(tiles=-1), b"tiles=-1"),
                           (clip, dict(tiles=2 ** 24 + 1), b"tiles=16777217"), (clip, dict(mx=0.0), b"max_norm"), (clip, dict(mx=-1.0), b"max_norm"),
                           (clip, dict(mx=nan), b"max_norm"), (clip, dict(ws=ctypes.c_void_p(4100)), b"8-byte aligned"),
                           (appl, dict(wd=N), b"optim_sgd_apply: null pointer"), (appl, dict(t=0), b"num_tensors=0"),
                           (appl, dict(tiles=2 ** 24 + 1), b"tiles="), (appl, dict(lr=nan), b"lr="), (appl, dict(lr=inf), b"lr="),
                           (appl, dict(mom=1.0), b"momentum="), (appl, dict(mom=-0.1), b"momentum="), (appl, dict(mom=nan), b"momentum="),
                           (appl, dict(mode=3), b"mode=3"), (appl, dict(mode=-1), b"mode=-1")):
        rc = call(**kw)
        assert rc == -1 and text in lib.mrcnn_last_error(), (text, rc, lib.mrcnn_last_error())
    assert appl(tiles=0) == 0      # nothing to do: no launch
