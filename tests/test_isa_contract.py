"""The inline-asm contracts of the hand-scheduled kernels, re-derived from the generated code (hipcc -S; no GPU): tools/isa_audit.py.

hipcc neither counts nor pads what is inside an asm string. conv3x3_wino4_f32 has asm MFMAs the hazard recogniser cannot see,
asm LDS reads behind hand-counted lgkmcnt(N) and staging waits vmcnt(3) counted by hand; conv_f16p has asm ds_read_b128 and counted
vmcnt(N); crop_forward_nchw_staged has asm ds_read2_b32 behind a counted lgkmcnt(8) and a run-time vmcnt budget on a 16-arm ladder
of asm waits. Round 6 met both failure modes this guards against: a build whose register allocation copied an accumulator 6 wait
states behind an asm MFMA (wrong sums; check C) and compiler copies of a[0:15] at the head of the k loop (check D)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_audit  # noqa: E402


@pytest.mark.parametrize("source", sorted(isa_audit.SOURCES))
def test_asm_contracts_hold(source):
    rep = isa_audit.audit_source(source)
    assert rep, f"{source}: no kernel with an asm contract found — the audit is not looking at anything"
    for name, r in rep.items():
        assert not r["violations"], f"{source}: {name}: {r['violations'][:5]} (meta {r['meta']})"
    if source == "conv_wino4.hip":
        assert len(rep) == 5   # plain (act / no act), heads (act / no act), conv2 + conv3
        for name, r in rep.items():
            # 4 waves x 2 k tiles of the loop x 36 MFMAs; every LDS-DMA of a k tile behind a hand-counted wait
            assert r["asm_mfma"] == 288 and r["asm_lds_reads"] >= 4 * (25 + 18) * 3 and r["asm_vmcnt_waits"] >= 12, (name, r)
    if source == "crop.hip":
        import crop_staged_cases as cc
        assert len(rep) == 1 and "crop_forward_nchw_staged" in next(iter(rep))
        r = next(iter(rep.values()))
        # two channels in flight + the odd one: 3 x 8 asm reads; 16 asm waits, all of them the ladder's; and the ladder the
        # generated code holds is the one the host restatement (tests/crop_staged_cases.py) counts arms with
        assert r["asm_lds_reads"] == 24 and r["asm_vmcnt_waits"] == 16 and r["lds_dma"] >= 8, r
        assert r["ladders"] == [[(a, a) for a in cc.LADDER]], r["ladders"]


def test_every_source_is_compiled_with_the_product_builds_flags():
    """crop.hip's arithmetic is built with FP contraction off; audited with other flags, the code looked at would not be the code
    that ships."""
    assert "-ffp-contract=off" in isa_audit.build_flags("crop.hip")
    assert isa_audit.build_flags("conv_f16p.hip") == []
    for source in isa_audit.SOURCES:
        isa_audit.build_flags(source)      # a KeyError: an audited source the product build does not know


def test_every_hand_scheduled_source_is_audited():
    """A csrc/*.hip whose inline asm holds a counted vector-memory wait, an LDS read or an MFMA takes a contract over from the
    compiler: it has to be in the audit's SOURCES. (Comments do not count; string literals in a file that uses asm do.)"""
    hand = set()
    for f in sorted(os.listdir(isa_audit.CSRC)):
        if not f.endswith(".hip"):
            continue
        text = open(os.path.join(isa_audit.CSRC, f)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        if not re.search(r"\basm\b", text):
            continue
        if any(re.search(r"s_waitcnt vmcnt|ds_read|v_mfma", lit) for lit in re.findall(r'"((?:[^"\\\n]|\\.)*)"', text)):
            hand.add(f)
    assert {"conv_wino4.hip", "conv_f16p.hip", "crop.hip"} <= hand, hand      # the scan sees the ones that are known
    assert hand <= set(isa_audit.SOURCES), f"hand-scheduled sources outside the audit: {sorted(hand - set(isa_audit.SOURCES))}"


def test_broken_contracts_are_reported():
    """Edits of the generated code that break ONE contract each (conv_wino4: a staging wait one too loose, a spill of an asm load's
    destination before its wait, an accumulator read behind an asm MFMA, a counted LDS wait one too loose, a compiler copy of
    a live accumulator inside the k loop; crop: lgkmcnt(8) -> lgkmcnt(9), a spill of an asm read's destination, a ladder arm
    that waits with more than its guard — out of order, in order, and the last arm): the audit must report every one — a test
    that cannot fail proves nothing."""
    assert set(isa_audit.MUTATIONS) == {"conv_wino4.hip", "crop.hip"}
    for source in sorted(isa_audit.MUTATIONS, reverse=True):      # crop.hip first: its audit takes a fraction of a second
        text = isa_audit.compile_asm(source)
        for what, (check, mutated) in isa_audit.MUTATIONS[source](text).items():
            assert mutated != text, (source, what)
            rep = isa_audit.audit_source(source, mutated)
            fired = {v[0] for r in rep.values() for v in r["violations"]}
            assert check in fired, f"{source}: mutation '{what}' not reported (checks that fired: {sorted(fired)})"
            if source == "crop.hip":
                assert fired == {check}, f"{source}: mutation '{what}': {sorted(fired)} fired, {check} expected alone"
