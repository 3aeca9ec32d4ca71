"""CPU checks of the exact-arithmetic conv sweep (tests/conv_exact_cases.py): the inputs make bit equality a theorem, the
float64 reference agrees with an independent int64 evaluation, and the fp32 cases reach every route of the dispatcher —
asked of the dispatcher itself through ops.conv_route, on a machine without a GPU."""
import collections
import itertools

import numpy as np
import pytest

import conv_exact_cases as C

CUS = 256   # MI355X

# Every route run_conv_f32 can take in a product build, written out by hand from conv_route_f32 (csrc/conv.hip). One line per
# (kernel, tile, split): the modes and epilogues that reach it. The 2x2 scatter (epilogue "scatter") comes from deconv2x2
# only — a 1x1 unpadded GEMM — so it never meets the aligned-tap mode; SPLIT needs K >= 1024, no generic K and an epilogue
# of 0-2 on one of three tiles; the streaming kernel takes plain pointwise calls only.
ALL, NO_GENERIC = ("aligned", "generic", "pointwise"), ("aligned", "pointwise")
EPI, EPI_SPLIT = ("plain", "residual", "residual_half", "sigmoid", "scatter"), ("plain", "residual", "residual_half")
REACHABLE = [
    # kernel, tile, split, modes, epilogues
    ("tiled", "128x32k32", False, ALL, EPI),              # cout <= 32
    ("tiled", "128x32k32", True, NO_GENERIC, EPI_SPLIT),  # cout <= 32 with K >= 1024; or underfilled && K >= 1024 && 128x64 tiles <= cus
    ("tiled", "256x64k32", False, ("generic",), EPI),     # 32 < cout <= 64, generic
    ("tiled", "256x64k16", False, NO_GENERIC, EPI),       # 32 < cout <= 64, cin % 32 == 0
    ("tiled", "128x96k32", False, NO_GENERIC, EPI),       # !generic && 64 < cout <= 96
    ("tiled", "128x128k16", False, NO_GENERIC, EPI),      # !generic && ((K <= 128 && cout >= 256) || (scatter && K <= 256 && cout >= 256))
    ("tiled", "128x64k16", False, NO_GENERIC, EPI),       # !generic && (underfilled || (K <= 256 && residual && res_div == 1 && cout >= 128))
    ("tiled", "128x64k16", True, NO_GENERIC, EPI_SPLIT),  # the same with K >= 1024 (underfilled, more than cus 128x64 tiles)
    ("tiled", "128x128k32", False, ALL, EPI),             # the rest: generic with cout > 64, 96 < cout < 128, or enough tiles for every CU
    ("tiled", "128x128k32", True, NO_GENERIC, EPI_SPLIT), # the rest with K >= 1024
    ("stream_256_64", None, False, ("pointwise",), ("plain",)),   # M >= 131072, cin == 256, 32 < cout <= 64
    ("stream_64_64", None, False, ("pointwise",), ("plain",)),    # M >= 131072, cin == 64, 32 < cout <= 64
    ("stream_64_256", None, False, ("pointwise",), ("plain",)),   # M >= 131072, cin == 64, 128 < cout <= 256
]


def reachable_routes():
    from maskrcnn_amd import ops
    out = set()
    for kernel, tile, split, modes, epis in REACHABLE:
        for mode, epi in itertools.product(modes, epis):
            if epi == "scatter" and mode == "aligned":
                continue
            out.add(ops.ConvRoute(kernel, tile, mode, epi, split))
    return out


def coverage_problems(cases, cus):
    """What is wrong with the coverage of the fp32 table on a device of `cus` CUs ([] = nothing): routes not reached, routes
    reached by fewer than two cases, routes reached that the hand-written table does not know."""
    from maskrcnn_amd import ops
    reached = collections.Counter(C.route_of(c, cus, ops) for c in cases)
    want = reachable_routes()
    return ([f"not reached: {r}" for r in sorted(want - set(reached), key=str)] +
            [f"reached once: {r}" for r, n in sorted(reached.items(), key=str) if n < 2 and r in want] +
            [f"not in the table: {r}" for r in sorted(set(reached) - want, key=str)])


ALL_CASES = C.fp32_cases(CUS) + C.f16mfma_cases() + C.f16io_cases() + C.f16p_cases()


def test_every_case_passes_its_invariants():
    ties = unrep = 0
    for case in ALL_CASES:
        d = C.build(case)
        C.check_invariants(case, d)
        if case.y16:
            t, u = C.f16_ties_and_unrepresentable(d.want)
            ties, unrep = ties + t, unrep + u
    # the fp16 outputs test the rounding, not just representable values
    assert ties >= 100 and unrep >= 100, (ties, unrep)


def test_case_table_covers_what_the_issue_lists():
    f32 = [c for c in ALL_CASES if c.op == "f32"]
    assert {c.k for c in f32} >= {1, 3, 5, 7} and any(c.stride == 2 for c in f32)
    assert {c.pad for c in f32} >= {(1, 1, 1, 1), (0, 0, 1, 1), (3, 3, 3, 3)}
    assert {c.res_kblocked for c in f32 if c.res} == {False, True}
    assert any(c.out_mode == 2 and c.shape != "pow2" for c in f32)                               # k-blocked output, ragged map
    assert any(c.res == 2 and c.out_hw == C.RAGGED_EVEN for c in f32)                             # division decode with res_div 2
    assert any(c.res and c.cout % 2 for c in f32)                                                # odd Cout with a residual
    assert any(c.out_mode == 1 and c.m % 128 and c.cout % 128 for c in f32)                      # deconv2x2, ragged M and N
    for c in f32:
        if c.rows:
            per, counts = c.rows
            assert 0 in counts and per in counts and any(0 < n < per for n in counts) and per * len(counts) == c.m
    assert sum(1 for c in f32 if c.rows) >= 2
    for c in ALL_CASES:
        if c.shape == "ragged" and c.op == "f32" and not c.family.startswith("stream"):
            assert c.b == 3 and c.m % 128 and all(v & (v - 1) for v in c.out_hw), c.id
    assert {c.tile for c in ALL_CASES if c.op == "f16p"} == set(C.F16P_TILES)
    io = {(c.x16, c.y16, c.epi, c.mode) for c in ALL_CASES if c.op == "f16io"}
    assert io == ({(False, True, 0, 0), (False, True, 0, 1)} | {(True, True, e, 0) for e in (0, 1, 2, 4)} |
                  {(True, False, e, 0) for e in (0, 3)})
    mf = {(c.products, c.cout <= 64, c.mode, c.epi) for c in ALL_CASES if c.op == "f16mfma"}
    assert mf == set(itertools.product((1, 3), (True, False), (0, 1), range(5)))


@pytest.mark.parametrize("name", ["t256x64_k32-m1e0-ragged", "t128x96-m0e2-ragged", "t128x32_split-m2e1-pow2"])
def test_float64_reference_equals_an_int64_evaluation(name):
    case = next(c for c in ALL_CASES if c.id == name)
    d = C.build(case)
    pre2 = C.int64_reference(case, d)
    assert np.array_equal(pre2.astype(np.float64), 2.0 * d.pre)
    y2 = np.maximum(pre2, 0) if case.act == 1 else pre2
    assert np.array_equal(C.to_layout(case, y2.astype(np.float64)), 2.0 * d.want)


def test_fp32_cases_reach_exactly_the_reachable_routes():
    cases = C.fp32_cases(CUS)
    assert len(reachable_routes()) == 90
    assert coverage_problems(cases, CUS) == []
    # the cases that depend on the CU count follow it
    for cus in (64, 228, 304):
        assert coverage_problems(C.fp32_cases(cus), cus) == [], cus


def test_coverage_assertion_fails_when_a_family_is_removed():
    """The mutation check: the table less any one family leaves a route unreached or reached once."""
    cases = C.fp32_cases(CUS)
    families = sorted({c.family for c in cases})
    assert len(families) == 13
    for fam in families:
        rest = [c for c in cases if c.family != fam]
        assert coverage_problems(rest, CUS), f"the coverage assertion does not notice that {fam} is gone"
