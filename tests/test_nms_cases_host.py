"""tests/nms_cases.py on the host: the closed form, the numpy restatement and the C oracle agree on every case; the data are
exact; the constructions reach what they claim (the 64-round fixpoint, the lane-63 / lane-0 and lane-31 / lane-32 hand-offs, dead
boxes with victims at every chunk distance, pairs exactly on the threshold); the case list reaches every plan the launcher can
produce; and every mutant of the restatement changes some case. tests/test_gpu_nms_edges.py runs the same cases on the kernels."""
import numpy as np
import pytest
import torch

import nms_cases as nc
from nms_cases import f32, f64

CASES = nc.all_cases()
STEPWISE_MAX = 4097          # nms_stepwise is O(kept x n): above this the closed form and the oracle suffice
T = {f32: torch.float32, f64: torch.float64}


def _dtypes(case):
    return (f32, f64) if "gen64" in case.paths else (f32,)


def _oracle(oracle, case, dtype):
    cls = None if case.class_ids is None else torch.from_numpy(case.class_ids)
    return oracle.nms(torch.from_numpy(case.dets).to(T[dtype]), case.thr, cls).numpy()


@pytest.fixture(scope="module")
def live():
    from oracle import build_ref
    return build_ref.load()          # the reference's own compiled nms_cpu.cpp, or None where it is not built


@pytest.mark.parametrize("name", list(CASES))
def test_closed_form_stepwise_and_oracle_agree(oracle, live, name):
    case = CASES[name]
    for dtype in _dtypes(case):
        want = _oracle(oracle, case, dtype)
        closed = nc.expected_keep(case, dtype)
        assert closed is not None or case.n <= STEPWISE_MAX, "a case above STEPWISE_MAX needs a closed form"
        if closed is not None:
            assert np.array_equal(closed, want), (name, dtype.__name__, "closed form")
        if case.n <= STEPWISE_MAX:
            assert np.array_equal(nc.nms_stepwise(case.dets, case.thr, case.class_ids, dtype), want), (name, dtype.__name__)
        if live is not None and case.class_ids is None:
            # the reference orders with ATen's sort, which is not stable: it gets the same boxes with the visiting order spelled
            # out in distinct scores (n - rank), which leaves the answer as it is
            d = case.dets.copy()
            d[nc.visit_order(d), 4] = np.arange(case.n, 0, -1)
            assert np.array_equal(live.nms(torch.from_numpy(d).to(T[dtype]), case.thr).numpy(), want), (name, dtype.__name__, "live")


def test_fp64_boxes_against_a_float_threshold():
    """(13, 7) chains at 0.3: fp32 keeps alternate chain elements, fp64 keeps every box (0.3 < (double)0.3f); (17, 3) at 0.7 gives
    the same result in both types. A 66-box chain keeps 33 and 66."""
    for n in (321, 1089):
        c = nc.composite(n, 0.3)
        assert c.links(f32) and not c.links(f64)
        assert nc.expected_keep(c, f64).size == n > nc.expected_keep(c, f32).size
        c = nc.composite(n, 0.7)
        assert c.links(f32) and c.links(f64) and np.array_equal(nc.expected_keep(c, f32), nc.expected_keep(c, f64))
    chain = np.array([[0, 7 * k, 4, 7 * k + 12, 100 - k] for k in range(66)], f64)
    assert nc.nms_stepwise(chain, 0.3, dtype=f32).size == 33 and nc.nms_stepwise(chain, 0.3, dtype=f64).size == 66


# ------------------------------------------------------------------------------------------------------------ exactness
def _inter(a, b):
    """Integer intersection (with the +1 convention) of int64 box arrays."""
    w = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]) + 1
    h = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]) + 1
    return np.maximum(w, 0) * np.maximum(h, 0)


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if c.group in ("composite", "classes") and c.closed == "chains"])
def test_data_are_exact_and_only_chain_mates_intersect(name):
    """Integer coordinates below 2^20, sides at most 17 (areas, intersections, unions far below 2^24), boxes of different chains
    disjoint — brute force up to 4097 boxes, above that by the row bands — and inside a chain the IoU of k-th neighbours is
    (w - k s) / (w + k s): on the threshold for k = 1, strictly below it for every k > 1."""
    case = CASES[name]
    b = case.dets[:, :4].astype(np.int64)
    assert np.array_equal(b, case.dets[:, :4]) and np.abs(b).max() < 2 ** 20
    assert np.array_equal(case.dets.astype(f32).astype(f64), case.dets)
    side_w, side_h = b[:, 3] - b[:, 1] + 1, b[:, 2] - b[:, 0] + 1
    assert side_w.min() >= 1 and side_h.min() >= 1 and side_w.max() <= 17 and side_h.max() <= 17
    chain_of = np.empty(case.n, np.int64)
    for cid, ch in enumerate(case.chains):
        chain_of[ch] = cid
    band = b[:, 0] // nc.BAND
    assert np.array_equal(band, (b[:, 2]) // nc.BAND)                                  # a box stays inside its band
    if case.class_ids is None:
        first = {}
        for i in range(case.n):                                                        # one chain per band
            assert first.setdefault(int(band[i]), int(chain_of[i])) == chain_of[i]
    if case.n <= 4097:
        for i in range(case.n):
            hit = np.flatnonzero(_inter(b[i], b) > 0)
            mates = hit[chain_of[hit] == chain_of[i]] if case.class_ids is None else hit[band[hit] == band[i]]
            assert mates.size == hit.size, (name, i)
    w, s = case.ws
    thr = float(f32(case.thr))
    assert (w - s) / (w + s) == pytest.approx(case.thr, abs=1e-7) and all((w - k * s) / (w + k * s) < thr - 0.01
                                                                         for k in range(2, w // s + 1))
    for ch in case.chains:                                                             # elements are s apart, same rows
        c = b[ch]
        assert (np.diff(c[:, 1]) == s).all() and (c[:, 0] == c[0, 0]).all() and (side_w[ch] == w).all()


# --------------------------------------------------------------------------------------------------------------- reached
def _simulate(case, dtype=f32):
    """The kernels' chunked resolution by integer logic on the sorted order. → kept [n] by sorted position, per chunk the rounds
    nms_scan_kernel's ballot fixpoint runs (the confirming round included) and the lanes the serial walk of nms_kernel /
    nmsg_chunk_kernel visits, and prev (earlier chain neighbours of every position)."""
    n = case.n
    order = nc.visit_order(case.dets)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    prev = [[] for _ in range(n)]
    if case.links(dtype):
        for ch in case.chains:
            for a, b in zip(ch[:-1], ch[1:]):
                lo, hi = sorted((int(pos[a]), int(pos[b])))
                prev[hi].append(lo)
    kept = np.zeros(n, bool)
    rounds, walked = [], []
    for c0 in range(0, n, 64):
        lanes = range(c0, min(c0 + 64, n))
        alive = {p: not any(kept[q] for q in prev[p] if q < c0) for p in lanes}
        k = dict(alive)
        for r in range(1, 66):
            nxt = {p: alive[p] and not any(k[q] for q in prev[p] if q >= c0) for p in lanes}
            if nxt == k:
                break
            k = nxt
        else:
            raise AssertionError("the fixpoint did not settle in 65 rounds")
        for p in lanes:                                                                # the greedy walk gives the same set
            kept[p] = alive[p] and not any(kept[q] for q in prev[p] if q >= c0)
            assert kept[p] == k[p]
        rounds.append(r)
        walked.append(int(sum(k.values())))
    return kept, rounds, walked, prev, order


def test_what_the_constructions_reach(capsys):
    depth = {}
    for name, case in CASES.items():
        if case.group != "composite":
            continue
        kept, rounds, walked, prev, order = _simulate(case)
        assert np.array_equal(np.sort(order[kept]), nc.expected_keep(case)), name
        plan = "lds columns" if case.n <= 1088 else "L2 columns"
        depth[name] = (max(rounds), max(walked), plan if "ws" in case.paths else "-")
        m, n = case.marks, case.n
        on_thr = sum(len(p) for p in prev)
        links = sum(len(ch) - 1 for ch in case.chains)
        assert on_thr == links and (on_thr >= 100 if n >= 257 else True), (name, on_thr)     # pairs exactly on the threshold
        a = m.get("chain_a", ())
        assert all(kept[p] == (p % 2 == 1) for p in a), name                            # chain A: the odd positions
        if n >= 65:
            assert kept[63] and not kept[64] and prev[64] == [63], name               # kept lane 63 kills lane 0 of the next chunk
        for c0 in (0, 64, 128):
            if n > c0 + 32:
                assert kept[c0 + 31] and not kept[c0 + 32] and prev[c0 + 32] == [c0 + 31], name   # kept lane 31 kills lane 32
        b = m.get("chain_b", ())
        assert all(kept[p] == (p % 2 == 0) for p in b), name
        if len(b) >= 64:
            assert rounds[4] == 64 and walked[4] >= 32, name                           # 64 alive lanes, each killing its successor
            assert kept[286] and not kept[287] and prev[287] == [286], name            # kept lane 30 kills lane 31
        if len(b) >= 65:
            assert not kept[319] and kept[320] and prev[320] == [319], name            # dead lane 63, surviving lane 0
        for key, p in m.items():
            if key.startswith("triple"):
                kk, d, e = p
                assert kept[kk] and not kept[d] and kept[e] and prev[e] == [d] and prev[d] == [kk], (name, key)
            elif key.startswith("pair"):
                h, s = p
                assert kept[h] and not kept[s] and prev[s] == [h], (name, key)
    with capsys.disabled():
        print()
        for name, (r, w, plan) in depth.items():
            print(f"  {name}: deepest chunk {r} fixpoint rounds, longest serial walk {w} lanes, scan {plan}")
    for plan in ("lds columns", "L2 columns"):
        assert max(r for r, _, p in depth.values() if p == plan) == 64, plan
    assert max(w for _, w, _ in depth.values()) >= 32
    # named cases
    big = CASES["composite-n2049-thr0.5"].marks
    dist = lambda key: big[key][-1] // 64 - big[key][0] // 64
    assert [dist(f"triple_{t}") for t in (0, 1, 7, 8, 9, 17)] == [0, 1, 7, 8, 9, 17] == [dist(f"pair_{t}") for t in (0, 1, 7, 8, 9, 17)]
    assert [dist(f"triple_6+{t}") for t in (1, 8, 9)] == [1, 8, 9] == [dist(f"pair_6+{t}") for t in (1, 8, 9)]
    assert big["pair_lane63_lane0"] == (703, 704) and big["pair_last"][1] == 2048 and big["pair_last"][0] < 64
    full = CASES["composite-n2048-thr0.5"].marks
    assert full["pair_last"][1] // 64 == full["triple_last"][2] // 64 == 2047 // 64
    g = CASES["composite-n321-thr0.5"].marks                     # general path, chunk 0's launch: blocks 64 .. 319 and 320 ..
    assert g["pair_last"][1] == 320 and g["pair_last"][0] < 64 and len(g["chain_b"]) == 64
    assert {CASES[f"composite-n{n}-thr0.5"].n % 64 for n in (1024, 1025, 63)} == {0, 1, 63}
    for name in ("composite-n321-thr0.5", "composite-n1089-thr0.5"):
        assert len(CASES[name].marks["tie_runs"]) >= 4


def test_segment_cases_rows_behind_the_count_would_matter(oracle):
    """Each segment's closed form equals the oracle on its first count rows; the oracle on ALL rows gives something else."""
    for n_max in (130, 300, 1089):
        seg = nc.segments_case(n_max)
        keep, cnt = seg.expected()
        assert cnt.tolist()[1:3] == [0, 1] and (keep[1] == -1).all()
        for s, c in enumerate(seg.counts):
            rows = torch.from_numpy(seg.dets[s]).float()
            assert np.array_equal(seg.dets[s, :c].astype(f32).astype(f64), seg.dets[s, :c])
            assert np.array_equal(oracle.nms(rows[:c], seg.thr).numpy(), keep[s, :cnt[s]]), (n_max, s)
            if c < n_max:
                assert not np.array_equal(oracle.nms(rows, seg.thr).numpy(), keep[s, :cnt[s]]), (n_max, s)


# ----------------------------------------------------------------------------------------------------------------- plans
def test_the_cases_reach_every_plan_of_the_launcher():
    """The table of reachable plans is the launcher's own answer (ops.nms_plan) over every n_max, with and without a workspace."""
    from maskrcnn_amd import _lib, ops
    assert _lib.header_abi_version() >= 37 and int(_lib.lib.mrcnn_abi_version()) == _lib.header_abi_version()
    reachable = {ops.nms_plan(n, True) for n in range(1, nc.NMS_MAX_WS + 1)} | \
                {ops.nms_plan(n, False) for n in range(1, nc.NMS_MAX_LDS + 1)}
    reached = set()
    for case in CASES.values():
        for path in case.paths:
            if path in ("lds", "ws"):
                plan = ops.nms_plan(case.n, path == "ws")
                assert plan.path == {"lds": "lds", "ws": "workspace"}[path], (case.name, plan)
                reached.add(plan)
    print(sorted(reachable))
    assert reached == reachable and len(reachable) == 10
    P = ops.NmsPlan
    assert ops.nms_plan(128, True) == P("lds", 256, 256, False) and ops.nms_plan(129, True) == P("workspace", 1024, 1024, True)
    assert ops.nms_plan(1088, True) == P("workspace", 2048, 1024, True) and ops.nms_plan(1089, True) == P("workspace", 2048, 1024, False)
    assert ops.nms_plan(256, False) == P("lds", 256, 256, False) and ops.nms_plan(257, False) == P("lds", 1024, 1024, False)
    for bad in ((0, True), (16385, True), (4097, False), (0, False)):
        with pytest.raises(ops.MaskrcnnHipError):
            ops.nms_plan(*bad)


# --------------------------------------------------------------------------------------------------------------- mutants
# A mutant no input can tell from the original. fmax / fmin differ from the `a < b ? b : a` ternaries only where a coordinate is
# NaN; every coordinate of a box enters its area, so the area is NaN, the union is NaN, inter / NaN is NaN and `NaN >= thr` is
# false under either rule: a box with a NaN coordinate neither suppresses nor is suppressed. (The asymmetry is real one step
# earlier — the clipped corner is NaN under the ternary and finite under fmax — but no keep set can show it.)
EQUIVALENT = ("symmetric_nan",)


def test_the_ternaries_keep_the_kept_boxes_nan_and_drop_the_candidates():
    """The one place where the asymmetry of the ternaries is visible: the clipped corner itself."""
    nan, one = f32("nan"), f32(1)
    kept_nan = (np.array([0, 0], f32), np.array([nan, 3], f32), np.array([4, 4], f32), np.array([9, 9], f32))
    cand_nan = (np.array([0, 0], f32), np.array([2, nan], f32), np.array([4, 4], f32), np.array([9, 9], f32))
    for b in (kept_nan, cand_nan):
        x1 = b[1]
        assert np.isnan(np.where(x1[0] < x1[1:], x1[1:], x1[0])[0]) == (b is kept_nan)       # std::max(ix1, x1[j])
        assert not np.isnan(np.fmax(x1[0], x1[1:])[0])
        area = ((b[3] - b[1]) + one) * ((b[2] - b[0]) + one)
        with np.errstate(invalid="ignore"):
            for mutant in (None, "symmetric_nan"):
                assert not nc._hits(0, np.array([1]), b, area, f32(0.0), one, mutant)[0]


def test_every_mutant_of_the_restatement_changes_some_case(capsys):
    small = [c for c in CASES.values() if c.n <= 321]
    right = {(c.name, d): nc.nms_stepwise(c.dets, c.thr, c.class_ids, d) for c in small for d in _dtypes(c)}
    killed = {}
    for mutant in nc.MUTANTS:
        killed[mutant] = [f"{name}/{d.__name__}" for (name, d), want in right.items()
                          if not np.array_equal(nc.nms_stepwise(CASES[name].dets, CASES[name].thr, CASES[name].class_ids, d, mutant), want)]
    with capsys.disabled():
        print()
        for mutant, names in killed.items():
            print(f"  mutant {mutant}: changes {len(names)} of {len(right)} runs, e.g. {names[:2]}")
    assert all(v for m, v in killed.items() if m not in EQUIVALENT), [m for m, v in killed.items() if not v]
    assert not any(killed[m] for m in EQUIVALENT)          # a case that tells one apart would belong to the list above
