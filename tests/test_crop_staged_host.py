"""The staged crop kernel's host restatement and launch table (tests/crop_staged_cases.py), checked without a GPU: the set of ring
regimes the kernel can meet is recomputed by enumeration, the launcher itself (ops.crop_plan) is asked for every launch's route,
every constructed box is put through the footprint restatement, the wait budget is replayed against the order in which the kernel
issues its vector-memory operations, and the two reciprocal-division claims of csrc/crop.hip are checked over their whole domains."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_staged_cases as cc  # noqa: E402


# ------------------------------------------------------------------------------------------------------- what can be reached
def test_reachable_arms_and_combinations_of_the_512_slot_ring():
    """By enumeration over S in 1..256, nchan in 1..16: the ladder arms 0..8, 10, 12, 14, a largest budget of 15 (so the arms 16, 20,
    24, 32 wait for a larger ring) and 18 (G, K, D). A change of the ring size or of the geometry changes this set: the table and
    this test then have to follow."""
    gkd, arms, top = cc.reachable()
    assert arms == set(range(9)) | {10, 12, 14}
    assert top == 15
    assert len(gkd) == 18
    assert {d for _, _, d in gkd} == {1, 3} and {k for _, k, _ in gkd} == {1, 2, 3, 4} and {g for g, _, _ in gkd} == set(range(1, 9))
    # what it takes: small launches (the launcher halves cpw while boxes x slabs < 4096) see the lower arms only
    for cpw, want in ((2, {0, 1, 2, 3, 4}), (4, set(range(7))), (8, set(range(9))), (16, set(range(9)) | {10, 12, 14})):
        assert cc.reachable(cpws=(cpw,))[1] == want, cpw
    for arm in (10, 12, 14):
        for S in range(1, 257):
            for nchan in range(1, 17):
                r = cc.ring_geometry(S, nchan)
                if arm in r.arms:
                    assert nchan >= 11 and r.K == 2 and r.ngroups >= 3, (arm, S, nchan)
    # a larger ring reaches further: the upper arms are not dead code
    assert cc.reachable(ring_slots=1024)[2] > 15


def test_arm_of_is_the_largest_immediate_not_above_the_budget():
    assert sorted(cc.LADDER, reverse=True) == list(cc.LADDER) and cc.LADDER[-1] == 0 and len(set(cc.LADDER)) == 16
    for n in range(0, 64):
        a = cc.arm_of(n)
        assert a in cc.LADDER and a <= n and not any(a < other <= n for other in cc.LADDER)


def test_ladder_in_the_source_is_the_restated_one():
    """cs_wait_vmcnt_at_most's `n >= C` / vmcnt(C) pairs, read from csrc/crop.hip: the guard and the immediate of every arm agree and
    the constants are LADDER's, in its order."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "maskrcnn_amd", "csrc", "crop.hip")).read()
    body = src[src.index("void cs_wait_vmcnt_at_most"):src.index("int cs_div_small")]
    arms = re.findall(r"if \(n >= (\d+)\) asm volatile\(\"s_waitcnt vmcnt\((\d+)\)\"", body)
    last = re.findall(r"else asm volatile\(\"s_waitcnt vmcnt\((\d+)\)\"", body)
    assert all(g == i for g, i in arms) and last == ["0"]
    assert tuple(int(g) for g, _ in arms) + (0,) == cc.LADDER


def test_geometry_in_the_source_is_the_restated_one():
    """The lines of crop_forward_nchw_staged that ring_geometry, first_of and the budget restate, word for word: a change of the
    kernel's geometry fails here until the restatement (and with it the table) follows. The GPU launches alone would not do:
    a wait that is too loose reads LDS the DMA may not have written yet, which on a quiet machine it usually has."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "maskrcnn_amd", "csrc", "crop.hip")).read()
    for line in ("constexpr int CS_RING_SLOTS = 512;",
                 "if (S > 256) {",
                 "const int BS = S <= 128 ? 128 : 256;",
                 "const int NB = ring_slots / BS;",
                 "const int G = min(min(8, cs_div_small(BS, S)), nchan);",
                 "const int K = (G * S + 63) >> 6;",
                 "const int D = NB - 1;",
                 "const int ngroups = cs_div_small(nchan + G - 1, G);",
                 "auto first_of = [&](int g) { return min(c_lo + g * G, depth - G); };",
                 "for (int g = 0; g < min(D, ngroups); ++g) dma(g, g);",
                 "if (g + D < ngroups) dma(g + D, buf_ahead);",
                 "const int ahead = min(D, ngroups - 1 - g);",
                 "cs_wait_vmcnt_at_most(ahead * K + min(D, g) * G);",
                 "const int gc = min(G, nchan - g * G);",
                 "const int shift = c_lo + g * G - first_of(g);"):
        assert src.count(line) == 1, line
    assert cc.RING_SLOTS == 512 and cc.MAX_STAGED_SLOTS == 256


@pytest.mark.parametrize("ring_slots", [512, 1024])
def test_budget_is_the_count_of_operations_issued_behind_the_group(ring_slots):
    """The kernel's issue order replayed: D groups' DMA pieces up front; then per group g the pieces of group g + D, the wait, and one
    store per channel. The budget the kernel computes must be EXACTLY the number of operations issued behind group g's last
    piece at the time of the wait (vector-memory operations retire in order: waiting for fewer is safe, for more reads LDS the
    DMA has not written), and the arm taken never exceeds it."""
    for S in range(1, 257):
        for nchan in range(1, 17):
            r = cc.ring_geometry(S, nchan, ring_slots)
            issued = []                       # ("dma", group) / ("store", group)
            for g in range(min(r.D, r.ngroups)):
                issued += [("dma", g)] * r.K
            for g in range(r.ngroups):
                if g + r.D < r.ngroups:
                    issued += [("dma", g + r.D)] * r.K
                last_piece = max(i for i, op in enumerate(issued) if op == ("dma", g))
                behind = len(issued) - 1 - last_piece
                assert r.budgets[g] == behind, (S, nchan, g, r)
                assert r.arms[g] <= behind
                # the buffer group g + D went into is the one group g - 1 was read from, and no other group in flight uses it
                assert len({h % r.NB for h in range(g, min(g + r.D, r.ngroups - 1) + 1)}) == min(r.D, r.ngroups - 1 - g) + 1
                issued += [("store", g)] * min(r.G, nchan - g * r.G)
            assert r.G * S <= r.BS and r.K <= 4 and r.NB * r.BS == ring_slots


def test_last_group_shift():
    """first_of keeps a group's G channels inside the image: a ragged last group whose G channels would end past the image's last
    channel starts that much early and skips the channels in front (in the last slab that is G - gc; a slab before a short last
    slab can need it too); otherwise it starts where it should and reads into the next slab's channels."""
    seen = set()
    for depth, cpw in ((31, 16), (15, 8), (13, 8), (7, 4), (5, 2)):
        for S in (1, 9, 17, 33, 65, 130):
            for slab in range(-(-depth // cpw)):
                c_lo = slab * cpw
                nchan = min(depth, c_lo + cpw) - c_lo
                r = cc.ring_geometry(S, nchan)
                gc = nchan - (r.ngroups - 1) * r.G
                shift = cc.last_shift(r, c_lo, depth)
                for g in range(r.ngroups):
                    f = cc.first_of(g, r.G, c_lo, depth)
                    assert 0 <= f and f + r.G <= depth
                assert shift == max(0, c_lo + r.ngroups * r.G - depth)
                if c_lo + nchan == depth:
                    assert shift == r.G - gc
                assert 0 <= shift and shift + gc <= r.G
                seen.add((shift > 0, c_lo + nchan == depth))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


# ------------------------------------------------------------------------------------------------------- the launcher's answer
def test_crop_plan_is_the_launchers_rule():
    from maskrcnn_amd import _lib, ops
    assert _lib.header_abi_version() >= 36 and int(_lib.lib.mrcnn_abi_version()) == _lib.header_abi_version()
    P = ops.CropPlan
    # channels per wave: 16 (8 on maps of 256 x 256 and more), halved while boxes x slabs < 4096, never below 2
    assert ops.crop_plan(256, 64, 64, 256, 14, 14) == P("staged", 16, 16, 1, 512, 8208)
    assert ops.crop_plan(256, 256, 256, 256, 14, 14) == P("staged", 8, 32, 1, 512, 8208)
    assert ops.crop_plan(31, 32, 32, 2048, 2, 2)[:4] == ("staged", 16, 2, 2)
    assert ops.crop_plan(31, 32, 32, 2047, 2, 2)[:4] == ("staged", 8, 4, 2)
    assert ops.crop_plan(7, 64, 64, 2048, 2, 4)[:4] == ("staged", 4, 2, 2)
    assert ops.crop_plan(7, 64, 64, 2047, 2, 4)[:4] == ("staged", 2, 4, 2)
    assert ops.crop_plan(1, 4, 4, 1, 2, 2)[:4] == ("staged", 2, 1, 2)
    assert ops.crop_plan(8, 256, 256, 4096, 2, 2)[:4] == ("staged", 8, 1, 2)
    assert ops.crop_plan(8, 252, 260, 4096, 2, 2)[:4] == ("staged", 16, 1, 2)        # 65520 pixels: below the rule
    # workgroup numbering: slabs % 8 == 0 -> 1, slabs in (1, 2, 4) -> 2, else the plain grid
    assert [ops.crop_plan(d, 64, 64, 10, 2, 2).map_mode for d in (2, 4, 6, 8, 10, 12, 14, 16, 18, 32)] == [2, 2, 0, 2, 0, 0, 0, 1, 0, 1]
    # the fallback's tap table may be larger than the ring
    assert ops.crop_plan(32, 64, 64, 128, 16, 16).lds_bytes == 16 * 32 + 32 * 256
    # what keeps a call off the staged kernel: plane % 4, plane > 256, ch + cw > 64, W % 4, alignment, 2^32 bytes per image,
    # more than 65535 slabs on the plain grid
    for args, kw in (((8, 64, 64, 10, 7, 7), {}), ((8, 64, 64, 10, 20, 20), {}), ((8, 64, 64, 10, 2, 64), {}),
                     ((8, 64, 62, 10, 2, 2), {}), ((8, 64, 64, 10, 2, 2), {"image": 4}), ((8, 64, 64, 10, 2, 2), {"crops": 8}),
                     ((256, 2048, 2048, 10, 2, 2), {}), ((16 * 65536 + 1, 1, 4, 1, 2, 2), {})):
        assert ops.crop_plan(*args, **kw).route == "gather", (args, kw)
    assert ops.crop_plan(8, 64, 64, 10, 2, 2, image=16, crops=32).route == "staged"
    assert ops.crop_plan(255, 2048, 2048, 10, 2, 2).route == "staged"
    assert ops.crop_plan(16 * 65536, 1, 4, 1, 2, 2)[:4] == ("staged", 16, 65536, 1)      # the 1-D grids have no such limit
    assert ops.crop_plan(16 * 65535 - 1, 1, 4, 1, 2, 2)[:4] == ("staged", 16, 65535, 0)
    # the gather kernel: ~2048 outputs per workgroup, at most 65535 slabs
    assert ops.crop_plan(300, 16, 16, 10, 3, 5) == P("gather", 137, 3, 0, 0, 16 * 8 + 32 * 15)
    assert ops.crop_plan(8, 64, 64, 10, 40, 40) == P("gather", 2, 4, 0, 0, 16 * 80)
    g = ops.crop_plan(16 * 65536 + 1, 1, 4, 1, 2, 2)
    assert g.slabs <= 65535 and g.cpw * g.slabs >= 16 * 65536 + 1
    for bad in ((0, 4, 4, 1, 2, 2), (1, 4, 4, 0, 2, 2), (1, 4, 4, 1, 0, 2), (1, 4, 4, 1, 2, 5000)):
        with pytest.raises(ops.MaskrcnnHipError):
            ops.crop_plan(*bad)


@pytest.mark.parametrize("launch", cc.LAUNCHES, ids=lambda l: l.id)
def test_launcher_gives_the_launch_the_route_it_names(launch):
    from maskrcnn_amd import ops
    assert os.environ.get("MRCNN_CROP_STAGED", "1") != "0"
    p = ops.crop_plan(launch.depth, launch.h, launch.w, launch.num_boxes, launch.ch, launch.cw)
    assert (p.route, p.cpw, p.slabs, p.map_mode, p.ring_slots) == ("staged", launch.cpw, launch.slabs, launch.map_mode, cc.RING_SLOTS)


# ------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("launch", cc.LAUNCHES, ids=lambda l: l.id)
def test_constructed_boxes_have_the_footprint_they_name(launch):
    seen = set()
    for b in cc.boxes_of(launch):
        if b in seen:
            continue
        seen.add(b)
        S = cc._crop_footprint_slots(b.coords, launch.h, launch.w, launch.ch, launch.cw)
        assert S == b.S, (b, S)
        ys = cc.samples(b.coords[0], b.coords[2], launch.h, launch.ch)
        xs = cc.samples(b.coords[1], b.coords[3], launch.w, launch.cw)
        inside = [i for i, _, _ in ys + xs]
        if b.kind in ("ring", "corner"):
            assert S <= cc.MAX_STAGED_SLOTS and all(inside)
        elif b.kind == "fallback":
            assert S > cc.MAX_STAGED_SLOTS
        elif b.kind == "outside":
            assert S is None and not any(i for i, _, _ in ys) and not any(i for i, _, _ in xs)
        elif b.kind == "partly":
            assert S <= cc.MAX_STAGED_SLOTS and any(inside) and not all(inside)
        if b.kind == "corner":
            assert {(lo, hi) for _, lo, hi in ys} == {(launch.h - 1,) * 2} and {(lo, hi) for _, lo, hi in xs} == {(launch.w - 1,) * 2}
    d = cc.build(launch)
    assert d["image"].dtype == np.float32 and d["boxes"].shape == (launch.num_boxes, 4) and d["index"].dtype == np.int32
    zeros = d["image"] == 0
    assert zeros.any() and np.signbit(d["image"][zeros]).all()
    assert ((d["index"] < 0) | (d["index"] >= launch.batch)).tolist() == d["bad"].tolist() and d["bad"].sum() >= 2
    assert ((d["valid_index"] >= 0) & (d["valid_index"] < launch.batch)).all()


def test_table_reaches_every_regime():
    assert cc.coverage_problems() == []
    gkd, arms = cc.reached()
    want_gkd, want_arms, _ = cc.reachable()
    assert gkd == want_gkd and arms == want_arms


def test_coverage_problems_notices_what_is_missing():
    by = {l.name: l for l in cc.LAUNCHES}

    def without(*names):
        return cc.coverage_problems([l for l in cc.LAUNCHES if l.name not in names])
    assert by.keys() >= {"cpw16-d31-48x32-2x2", "cpw8-d8-256x256-2x2"}
    p = without("cpw16-d31-48x32-2x2")
    assert {"missing: ladder arm 10", "missing: ladder arm 12", "missing: ladder arm 14", "missing: cpw 16"} <= set(p)
    assert "missing: (G, K, D) = (5, 1, 3)" in without("cpw8-d13-40x48-2x2")
    assert "missing: (G, K, D) = (6, 1, 3)" in without("cpw8-d14-64x64-7x8") and "missing: plane 56" in without("cpw8-d14-64x64-7x8")
    assert "missing: cpw 4" in without("cpw4-d7-64x64-2x4")
    assert "missing: map mode 0" in without("cpw2-d5-64x64-2x2-grid")
    assert "missing: plane 196" in without("cpw8-d31-64x64-14x14") and "missing: plane 256" in without("cpw2-d32-64x64-16x16")
    assert any("65536" in m for m in without("cpw8-d8-256x256-2x2"))
    assert "missing: map mode 2 with num_boxes no multiple of 8 / slabs" in without("cpw2-d3-64x64-4x4-ragged", "cpw8-d8-256x256-2x2")
    assert cc.coverage_problems([]) != []


# ------------------------------------------------------------------------------------------------------- the reciprocal claims
def test_cs_div_small_equals_integer_division():
    """cs_div_small(a, b) for a < 1024, 1 <= b <= a, with every value a 1-ulp reciprocal may take."""
    a = np.arange(1024, dtype=np.int64)[:, None]
    b = np.arange(1, 1024, dtype=np.int64)[None, :]
    domain = b <= a
    for r in cc.rcp_candidates(b):
        q = cc.div_by_reciprocal(a, r)
        assert (q == a // b)[domain].all()
    # the kernel's own uses lie inside the domain: BS / S with S <= BS, (nchan + G - 1) / G with G <= nchan <= 16
    assert all(1 <= S <= (128 if S <= 128 else 256) for S in range(1, 257))


def test_slot_and_position_splits_equal_integer_division():
    """slot -> (channel, row, segment): slot < 256 by S and the remainder (< S) by the segments per row; crop position p < 256 by
    the crop width: a < 256, 1 <= b <= 256 (b > a: quotient 0), with every value a 1-ulp reciprocal may take."""
    a = np.arange(256, dtype=np.int64)[:, None]
    b = np.arange(1, 257, dtype=np.int64)[None, :]
    for r in cc.rcp_candidates(b):
        q = cc.div_by_reciprocal(a, r)
        assert (q == a // b).all()
    # and the whole split, as the kernel composes it
    for S, nseg in ((1, 1), (12, 4), (21, 3), (65, 5), (130, 5), (196, 7), (256, 8)):
        for rS in cc.rcp_candidates(np.array([S])):
            for rseg in cc.rcp_candidates(np.array([nseg])):
                slot = np.arange(256)
                cg = cc.div_by_reciprocal(slot, rS[0])
                t = slot - cg * S
                row = cc.div_by_reciprocal(t, rseg[0])
                assert (cg == slot // S).all() and (row == (slot % S) // nseg).all() and ((t - row * nseg) == (slot % S) % nseg).all()
