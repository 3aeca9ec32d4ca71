"""CPU checks of the exact-arithmetic sweep over the fused kernels (tests/fused_exact_cases.py): for every case the conditions
that make bit equality with float64 a theorem (every sum and result fits fp32's 24 bits in any order), that make the case a
test (operands mostly non-zero, ReLUs that cut about half, fp16 intermediates that really round, ties included) and, per
family, that ONE thing done wrong in the reference changes the expected output: the data would notice that error in a kernel.
Run with -s for the ledger of every case (significant bits per sum, share of rounded values)."""
import numpy as np
import pytest

import fused_exact_cases as C
from conv_exact_cases import f16_ties_and_unrepresentable

_ID = lambda c: c.id
# the operands that must be mostly non-zero, per family (the stem's weights: the three real channels)
OPERANDS = {"wino": ("x", "w"), "heads": ("x", "w", "w_head32"), "block32": ("x", "w1", "w2", "w3"), "stem": ("img", "w"),
            "c2f16": ("x", "w1", "w2", "w3", "wd"), "tail": ("x", "wde", "w5")}


def _live(name, t):
    return t[:18] if name == "w_head32" else t[..., :3] if name == "w" and t.shape[1:] == (7, 7, 4) else t


@pytest.mark.parametrize("case", C.ALL_CASES, ids=_ID)
def test_case_is_exact_and_discriminating(case):
    d = C.build(case)
    fam = C.family_of(case)
    # exactness: sum |a||b| of every accumulation (for F(2x2): the absolute Winograd evaluation, granule 1/4) and the bound of
    # every affine / residual result, in granules, below 2^24
    bits = d.budget.bits()
    print(f"\n{case.id}: bits " + ", ".join(f"{k} {v:.1f}" for k, v in bits.items()))
    for name, v in bits.items():
        assert v < 24.0, (case.id, name, f"{v:.2f} bits: may not be exact in fp32")
    # operands: fp16 operands are fp16 values, fp32 results are fp32 values
    for name in d.f16_operands:
        t = getattr(d, name)
        assert np.array_equal(t.astype(np.float16).astype(np.float64), t), (case.id, name, "is not an fp16 value")
    if fam == "tail":
        assert np.array_equal(d.pre.astype(np.float32).astype(np.float64), d.pre), (case.id, "the sigmoid's argument")
        inside = float((np.abs(d.pre) <= 6).mean())
        print(f"    sigmoid arguments in [-6,6]: {inside:.3f}")
        assert inside >= 0.5, (case.id, inside)
    else:
        for w64, w in zip(*[v.values() if isinstance(v, dict) else (v,) for v in (d.want64, d.want)]):
            assert w.dtype == C.out_dtype(case)
            if w.dtype == np.float32:
                assert np.array_equal(w.astype(np.float64), w64), (case.id, "the expected output is not an fp32 value")
            assert np.isfinite(w).all() and not np.signbit(w[w == 0]).any(), (case.id, "inf or -0 in the expected output")
    # discrimination
    for name in OPERANDS[fam]:
        t = getattr(d, name, None)
        if t is not None:
            t = _live(name, t)
            assert np.count_nonzero(t) >= 0.3 * t.size, (case.id, name, "too many zeros")
    if fam == "heads":
        assert not d.w_head32[18:].any()
    if fam == "stem":
        assert not d.w[..., 3].any()
    for name, pre in d.relu_layers.items():
        cut = float((pre <= 0).mean())
        print(f"    {name}: {cut:.2f} <= 0 before the ReLU")
        assert 0.2 <= cut <= 0.8, (case.id, name, cut)
    for name, (exact, rounded) in d.rounded.items():
        changed = float((exact != rounded).mean())
        ties = f16_ties_and_unrepresentable(exact)[0] / exact.size
        print(f"    fp16 {name}: {changed:.3f} changed by the rounding, {ties:.4f} on a tie")
        assert np.isfinite(rounded).all() and float(np.abs(exact).max()) < 65504, (case.id, name)
        assert changed >= 0.10 and ties >= 0.01, (case.id, name, changed, ties)
    if getattr(case, "dead", False):     # all shifts far below: the ReLU map, the pool's padding and the result are +0
        assert float(d.pre.max()) < 0 and not d.want.any() and not np.signbit(d.want).any()


def _applies(case, mut):
    if getattr(case, "dead", False):
        return False        # that case is about zeros: every output is +0 whatever the mutant does
    if mut == "pool_pad_top_left":
        return case.op.startswith("pool") and case.h > 4      # one pooled pixel sees the whole 2 x 2 conv map either way
    if mut == "last_image":
        return (case.r if C.family_of(case) == "tail" else case.b) > 1
    return True


def _want(d):
    return np.concatenate([v.ravel() for v in d.values()]) if isinstance(d, dict) else d


@pytest.mark.parametrize("family", sorted(C.FAMILIES), ids=str)
def test_mutants_of_the_reference_change_the_expected_output(family):
    """One thing wrong — two input channels swapped, a tap shifted by a pixel, the last image replaced by the first,
    truncation for round-to-nearest-even on each rounding fp16 intermediate, the residual added after the ReLU, edge replication
    for the zero padding, the pool's pad on the wrong side — and at least one element of `want` differs, in every case of the
    family to which the mutant applies (and it applies to at least one)."""
    cases, _, operands, evaluate, xname, muts = C.FAMILIES[family]
    seen = {}
    for case in cases:
        d = C.build(case)
        o = operands(case)
        ref = _want(evaluate(case, o)["want"])
        assert np.array_equal(ref, _want(d.want64 if family != "wino" else d.want64[(True, True)])), case.id
        names = [m for m in muts if m != "trunc"] + [f"trunc:{n}" for n in d.rounded] + ["swap_channels", "last_image"]
        for mut in names:
            if not _applies(case, mut):
                continue
            if mut == "swap_channels":
                o2 = dict(o)
                o2[xname] = np.ascontiguousarray(o[xname][..., [1, 0] + list(range(2, o[xname].shape[-1]))])
                got = evaluate(case, o2)["want"]
            elif mut == "last_image":
                o2 = dict(o)
                o2[xname] = o[xname].copy()
                o2[xname][-1] = o[xname][0]
                got = evaluate(case, o2)["want"]
            else:
                got = evaluate(case, o, mut=mut)["want"]
            n = int((_want(got) != ref).sum())
            assert n > 0, f"{case.id}: the data do not notice the mutant {mut}"
            seen[mut] = seen.get(mut, 0) + 1
    want = {m for m in muts if m != "trunc"} | {"swap_channels", "last_image"}
    assert want <= set(seen), sorted(want - set(seen))
    if "trunc" in muts:
        assert any(m.startswith("trunc:") for m in seen), family
    print(f"\n{family}: " + ", ".join(f"{m} x{n}" for m, n in sorted(seen.items())))


def test_case_table_covers_what_it_promises():
    assert C.coverage_problems() == []
    ids = [c.id for c in C.ALL_CASES]
    assert len(set(ids)) == len(ids)
    # the assertion notices a missing shape, tiling, block kind or kernel form
    for gone in ("wino-spatial-1x32x16x512x64", "heads-f16p-3x13x11x64x512", "stem-conv_f16-2x38x70", "stem-pool_f16-2x24x36-dead",
                 "c2f16-first-1x5x3", "tail-7x14x14x2", "block32-1x16x16"):
        assert gone in ids
        assert C.coverage_problems([c for c in C.ALL_CASES if c.id != gone]), gone


@pytest.mark.parametrize("case", [c for c in C.WINO_CASES if c.cin <= 24], ids=_ID)
def test_the_conv_reference_equals_a_float64_f2x2_evaluation(case):
    """The transforms fused_exact_cases.wino_abs bounds are the ones that compute the convolution."""
    o = C.wino_operands(case)
    assert np.array_equal(C.wino64(o["x"], o["w"]), C.conv64(o["x"], o["w"], (1, 1, 1, 1)))


def test_the_deconv_reference_equals_conv_transpose2d():
    case = C.TAIL_CASES[0]
    o = C.tail_operands(case)
    assert np.array_equal(C.tail_eval(case, o)["de"], C.tail_deconv_torch(case, o))
