"""Constructed NMS inputs whose answer is known before any IoU is computed, and two references that share no code with the
kernels (csrc/nms.hip, csrc/nms_general.hip) or with oracle/nms_ref.c. No GPU and no oracle import here:
tests/test_nms_cases_host.py proves that the cases do what they claim, tests/test_gpu_nms_edges.py runs them.

Boxes are (y1, x1, y2, x2, score) with the reference's +1 convention. Every coordinate is an integer below 2^20, every width and
height at most 17: areas, intersections and unions are small integers, exact in fp32 and fp64, and the quotient is the only
operation that rounds.

The building block is the CHAIN. Element k of a chain of width w, step s, height h at origin (Y, X) is
(Y, X + k s, Y + h - 1, X + k s + w - 1): neighbours have IoU exactly (w - s) / (w + s), second neighbours (w - 2s) / (w + 2s)
(0 when 2s >= w). The three chain types put the neighbour IoU ON the threshold they are used with, every farther pair below it:

    (w, s)     neighbour   second      third      threshold
    (12, 4)    1/2         1/5         0          0.5
    (13, 7)    3/10        0           0          0.3
    (17, 3)    7/10        11/23       8/26       0.7

Every chain, and every isolated filler box (a chain of one), has a band of 32 rows to itself (Y = 32 * chain id, h <= 17), so two
boxes of different chains have intersection 0. A case gives every box a SORTED POSITION through its score and an input index
through a fixed permutation; elements of one chain may sit at any sorted positions. The answer follows by integer logic
(expected_keep): visit the boxes by (score descending, index ascending); a box that is not yet suppressed is kept and suppresses
its chain neighbours that come later. Whether a neighbour pair suppresses at all is one comparison of one correctly rounded
quotient of two small integers with the float threshold (Case.links): 3/10 against 0.3f is True in fp32 (fl32(3/10) == 0.3f) and
False in fp64 (0.3 < (double)0.3f), which is what separates `static_cast<T>(thr)` from a double threshold."""
import dataclasses
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64
CHAIN_TYPES = {0.5: (12, 4), 0.3: (13, 7), 0.7: (17, 3)}
BAND = 32                                    # rows per chain
COMPOSITE_SIZES = (1, 63, 64, 65, 128, 129, 256, 257, 321, 1024, 1025, 1088, 1089, 2048, 2049, 4096, 4097, 8192, 8193, 16384,
                   16385)
GENERAL_SIZES = (1, 64, 65, 321, 1089, 16385)          # every chunk of the general path is a launch
THREE_TYPE_SIZES = (321, 1089, 4097)                   # also built with (13, 7) at 0.3 and (17, 3) at 0.7
NMS_MAX_LDS, NMS_MAX_WS = 4096, 16384


def paths_for(n, general=None):
    """The implementations that take a single segment of n boxes: "lds" (nms_kernel), "ws" (sort / mask / scan), "gen32" / "gen64"
    (nms_general)."""
    general = n in GENERAL_SIZES if general is None else general
    p = []
    if n <= NMS_MAX_LDS:
        p.append("lds")
    if 128 < n <= NMS_MAX_WS:
        p.append("ws")
    if general:
        p += ["gen32", "gen64"]
    return tuple(p)


@dataclasses.dataclass
class Case:
    name: str
    dets: np.ndarray                 # float64 [n, 5]; every value is exact in float32 too
    thr: float                       # as a caller writes it (0.3); the kernels see float32(thr)
    paths: tuple
    class_ids: np.ndarray = None     # int32 [n] or None
    chains: list = None              # input indices of every chain in element order (None: no closed form)
    ws: tuple = None                 # (w, s) of the chains
    closed: str = None               # "chains" (walk the chains), "all" (everything kept), "first" (only the first visited), None
    marks: dict = dataclasses.field(default_factory=dict)    # name -> sorted positions the builder placed for it
    group: str = ""

    @property
    def n(self):
        return self.dets.shape[0]

    def links(self, dtype):
        """Does a chain-neighbour pair suppress in `dtype`? fl((w - s) / (w + s)) >= (dtype)(float)thr: one correctly rounded
        quotient of two small integers, the only rounding in these cases."""
        w, s = self.ws
        t = np.dtype(dtype).type
        return bool(t(w - s) / t(w + s) >= t(f32(self.thr)))


def visit_order(dets):
    """Input indices by (NaN scores first, score descending with -0 == +0, index ascending)."""
    s = np.asarray(dets)[:, 4].astype(f64)
    nan = np.isnan(s)
    return np.lexsort((np.arange(s.size), -np.where(nan, 0.0, s), ~nan))


def expected_keep(case, dtype=f32):
    """The closed form: integer logic on the chains, no IoU arithmetic. → ascending input indices (int64), or None."""
    n = case.n
    if case.closed is None:
        return None
    order = visit_order(case.dets)
    if case.closed == "first":
        return np.array([order[0]], dtype=np.int64)
    if case.closed == "all" or not case.links(dtype):
        return np.arange(n, dtype=np.int64)
    nb = [[] for _ in range(n)]
    for ch in case.chains:
        for a, b in zip(ch[:-1], ch[1:]):
            nb[a].append(b)
            nb[b].append(a)
    sup, seen = np.zeros(n, bool), np.zeros(n, bool)
    for i in order:
        seen[i] = True
        if not sup[i]:
            for j in nb[i]:
                if not seen[j]:
                    sup[j] = True
    return np.flatnonzero(~sup).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the second reference: nms_cpu.cpp restated in numpy, every operation rounded on its own in the boxes' type
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = ("gt", "no_plus_one", "dead_suppress", "dead_suppress_in_chunk", "ties_descending_index", "nan_last",
           "negative_zero_below", "classes_ignored", "symmetric_nan", "double_threshold", "fixpoint_8_rounds", "sign_extended_mask")


def _order(score, mutant):
    s = score.astype(f64)
    nan = np.isnan(s)
    idx = np.arange(s.size)
    key = -np.where(nan, 0.0, s)
    if mutant == "negative_zero_below":
        key = np.where((s == 0) & np.signbit(s), np.nextafter(0.0, 1.0), key)
    tie = -idx if mutant == "ties_descending_index" else idx
    return np.lexsort((tie, key, nan if mutant == "nan_last" else ~nan))


def _hits(i, js, b, area, thr, one, mutant):
    """ovr(i, j) >= thr for kept box i and candidates js, as nms_cpu.cpp:54-65: max / min are `a < b ? b : a` with the kept box as
    a, so a NaN of the kept box survives and a NaN of the candidate is replaced."""
    y1, x1, y2, x2 = b
    zero = one * 0
    if mutant == "symmetric_nan":
        xx1, yy1 = np.fmax(x1[i], x1[js]), np.fmax(y1[i], y1[js])
        xx2, yy2 = np.fmin(x2[i], x2[js]), np.fmin(y2[i], y2[js])
    else:
        xx1 = np.where(x1[i] < x1[js], x1[js], x1[i])
        yy1 = np.where(y1[i] < y1[js], y1[js], y1[i])
        xx2 = np.where(x2[js] < x2[i], x2[js], x2[i])
        yy2 = np.where(y2[js] < y2[i], y2[js], y2[i])
    tw, th = (xx2 - xx1) + one, (yy2 - yy1) + one
    w, h = np.where(zero < tw, tw, zero), np.where(zero < th, th, zero)
    inter = w * h
    ovr = inter / ((area[i] + area[js]) - inter)
    return ovr > thr if mutant == "gt" else ovr >= thr


def nms_stepwise(dets, thr, class_ids=None, dtype=f32, mutant=None):
    """Greedy NMS as cpu/nms_cpu.cpp:11-70 writes it, in `dtype`, operation by operation (numpy rounds each array operation
    separately). The threshold is a float converted to the box type. → ascending input indices of the survivors (int64).
    `mutant`: one of MUTANTS, a deliberately wrong variant (tests/test_nms_cases_host.py: every one must change some case)."""
    assert mutant is None or mutant in MUTANTS, mutant
    t = np.dtype(dtype).type
    d = np.asarray(dets).astype(t)
    n = d.shape[0]
    one = t(0) if mutant == "no_plus_one" else t(1)
    thr_t = t(thr) if mutant == "double_threshold" else t(f32(thr))
    cls = None if class_ids is None or mutant == "classes_ignored" else np.asarray(class_ids)
    order = _order(d[:, 4], mutant)
    with np.errstate(all="ignore"):
        b = tuple(d[order, c] for c in range(4))               # sorted order from here on
        area = ((b[3] - b[1]) + one) * ((b[2] - b[0]) + one)
        c = None if cls is None else cls[order]
        same = (lambda i, js: True) if c is None else (lambda i, js: c[js] == c[i])
        sup = np.zeros(n, bool)
        if mutant in ("fixpoint_8_rounds", "sign_extended_mask"):
            _resolve_by_chunks(n, b, area, thr_t, one, same, sup, mutant)
        else:
            for i in range(n):
                if sup[i] and mutant not in ("dead_suppress", "dead_suppress_in_chunk"):
                    continue
                hi = min(n, (i // 64 + 1) * 64) if (sup[i] and mutant == "dead_suppress_in_chunk") else n
                js = np.arange(i + 1, hi)
                sup[js] |= _hits(i, js, b, area, thr_t, one, mutant) & same(i, js)
    return np.sort(order[~sup]).astype(np.int64)


def _resolve_by_chunks(n, b, area, thr, one, same, sup, mutant):
    """The kernels' shape — 64-box chunks of the sorted order, a chunk's survivors suppress every later box — with one of two
    faults: the ballot fixpoint of nms_scan_kernel stopped after 8 rounds, or the serial walk of nms_kernel with the low word
    of a row's mask sign-extended into the high word."""
    for c0 in range(0, n, 64):
        m = min(64, n - c0)
        alive = ~sup[c0:c0 + m]
        hit = np.zeros((m, m), bool)                            # hit[i, j]: earlier lane i would suppress lane j
        for i in range(m - 1):
            js = np.arange(c0 + i + 1, c0 + m)
            hit[i, i + 1:] = _hits(c0 + i, js, b, area, thr, one, None) & same(c0 + i, js)
        if mutant == "fixpoint_8_rounds":
            kept = alive.copy()
            for _ in range(8):
                nxt = alive & ~(hit & kept[:, None]).any(0)
                if (nxt == kept).all():
                    break
                kept = nxt
        else:
            if m > 32:
                hit[hit[:, 31], 32:] = True                     # bit 31 of the low word smeared over the high word
            kept, al = np.zeros(m, bool), alive.copy()
            for i in range(m):
                if al[i]:
                    kept[i] = True
                    al &= ~hit[i]
        sup[c0:c0 + m] = ~kept
        for i in np.flatnonzero(kept) + c0:
            js = np.arange(c0 + m, n)
            sup[js] |= _hits(i, js, b, area, thr, one, None) & same(i, js)


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------
def _perm(n):
    """Sorted position -> input index: p -> (a p + n // 3) mod n with a near 0.618 n, coprime to n."""
    a = int(n * 0.6180339887) | 1
    while math.gcd(a, n) != 1:
        a += 2
    return (np.arange(n, dtype=np.int64) * a + n // 3) % n


class _Layout:
    """Sorted positions handed out to chains. place() takes all of a chain's positions or none."""

    def __init__(self, n):
        self.n, self.owner, self.chains, self.marks = n, [None] * n, [], {}

    def free(self, p):
        return 0 <= p < self.n and self.owner[p] is None

    def place(self, positions, mark=None):
        positions = list(positions)
        if not positions or len(set(positions)) != len(positions) or not all(self.free(p) for p in positions):
            return False
        cid = len(self.chains)
        self.chains.append(positions)
        for k, p in enumerate(positions):
            self.owner[p] = (cid, k)
        if mark:
            self.marks[mark] = tuple(positions)
        return True


def _finish(name, lay, w, s, thr, runs, paths, group, class_of_chain=None, same_place=None):
    """Fillers for the free positions, scores with the tie runs, the permutation, the boxes."""
    n = lay.n
    for p in range(n):
        if lay.owner[p] is None:
            lay.place([p])
    in_run = np.zeros(n, bool)
    for a, b in runs:
        if 1 <= a and b <= n and b - a >= 2 and not in_run[a - 1:b].any():
            in_run[a + 1:b] = True                               # position p shares the score of p - 1
            lay.marks.setdefault("tie_runs", []).append((a, b))
    level = np.cumsum(~in_run) - 1
    score = (level.max() + 1 - level).astype(f64)                # integers: exact in fp32
    order = _perm(n)
    for a, b in lay.marks.get("tie_runs", []):
        order[a:b] = np.sort(order[a:b])                          # equal scores are visited by ascending input index
    dets = np.zeros((n, 5), f64)
    cls = None if class_of_chain is None else np.zeros(n, np.int32)
    for p in range(n):
        cid, k = lay.owner[p]
        place = cid if same_place is None else same_place[cid]    # copies of one chain share its coordinates
        y, h, x = BAND * place, 1 + place % 17, k * s
        dets[order[p]] = (y, x, y + h - 1, x + w - 1, score[p])
        if cls is not None:
            cls[order[p]] = class_of_chain[cid]
    assert np.array_equal(visit_order(dets), order), name
    chains = [[int(order[p]) for p in ch] for ch in lay.chains]
    return Case(name, dets, thr, paths, cls, chains, (w, s), "chains", lay.marks, group)


@functools.lru_cache(maxsize=None)
def composite(n, thr=0.5, general=None):
    """The composite case of n sorted positions (see the module text for the chain types):
      0            an isolated box
      1 .. 200     chain A on every position but the slots 4 .. 27 and 66 .. 69 (even counts: its kept elements are the odd
                   positions). Kept lane 63 kills lane 0 of the next chunk, kept lane 31 kills lane 32 in chunks 0, 1 and 2.
      4 .. 27      K, D (triples) and H (pairs) whose victims sit in chunk 0, 1, 7, 8, 9, 17 and in the last chunk: a triple
                   K, D, E is a chain of three — K kills D, so E, which only D would kill, survives; a pair H, S — H kills S
      256 .. 330   chain B from lane 0 of chunk 4: kept elements are the even lanes, all 64 lanes alive when the chunk is resolved
                   (the 64-round fixpoint), kept lane 30 kills lane 31, lane 63 is dead and lane 0 of chunk 5 survives
      384 .. 447   K, D, H in chunk 6 with victims 1, 8 and 9 chunks later; H at lane 63 of chunk 10, S at lane 0 of chunk 11
    Positions that do not exist drop the chain that needs them. The rest are isolated fillers. Runs of sorted positions share a
    score; the input order is a fixed permutation of the sorted order."""
    w, s = CHAIN_TYPES[thr]
    lay = _Layout(n)
    lay.place([0])
    slots = iter(range(4, 28))

    def request(kind, tag, victim):
        """A triple (K, D in chunk 0, E = victim) or a pair (H in chunk 0, S = victim); victim None: in chunk 0 too."""
        if victim is not None and not lay.free(victim):
            return
        need = (2 if kind == "triple" else 1) + (victim is None)
        got = [next(slots) for _ in range(need)]
        lay.place(got if victim is None else got + [victim], f"{kind}_{tag}")

    if n > 202:                                                   # the last chunk first: nothing else may take its positions
        if n % 64 == 1:
            request("pair", "last", n - 1)                       # general path: the only active thread of the last block (n = 321)
        else:
            request("pair", "last", n - 1)
            request("triple", "last", n - 2)
    request("triple", "0", None)
    request("pair", "0", None)
    request("triple", "1", 66)
    request("pair", "1", 67)
    for t in (7, 8, 9, 17):
        request("triple", str(t), 64 * t + 5)
        request("pair", str(t), 64 * t + 6)
    reserved = set(range(4, 28)) | set(range(66, 70))
    if n > 1:
        lay.place([p for p in range(1, min(200, n - 1) + 1) if p not in reserved], "chain_a")
    b = []
    for p in range(256, min(331, n)):
        if not lay.free(p):
            break
        b.append(p)
    if len(b) >= 2:
        lay.place(b, "chain_b")
    for i, t in enumerate((1, 8, 9)):
        lay.place([394 + 2 * i, 395 + 2 * i, 64 * (6 + t) + 7], f"triple_6+{t}")
        lay.place([424 + i, 64 * (6 + t) + 8], f"pair_6+{t}")
    lay.place([64 * 10 + 63, 64 * 11], "pair_lane63_lane0")
    runs = [(40, 45), (62, 66), (100, 104), (258, 262), (n - 3, n)]
    return _finish(f"composite-n{n}-thr{thr}", lay, w, s, thr, runs, paths_for(n, general), "composite")


def with_threshold(case, thr, name, closed, group):
    """The same boxes under another threshold."""
    return dataclasses.replace(case, name=name, thr=thr, closed=closed, group=group)


def next_up(thr):
    return float(np.nextafter(f32(thr), f32(np.inf)))


@functools.lru_cache(maxsize=None)
def classes_case(n, copies, ids):
    """`copies` copies of one (12, 4) chain at the SAME coordinates, interleaved in sorted order (element k of copy c at position
    k * copies + c). ids "positive": copy c has class c + 1, each copy resolves on its own; "negative": pairwise distinct negative
    ids, as detection_decode writes for excluded slots — nothing suppresses anything; "none": no class_ids, judged by
    nms_stepwise (closed form undefined: identical boxes of different copies suppress each other)."""
    lay = _Layout(n)
    length = n // copies
    for c in range(copies):
        lay.place([k * copies + c for k in range(length)])
    n_chains = copies + (n - copies * length)
    same_place = [0] * copies + list(range(1, n_chains - copies + 1))
    case = _finish(f"classes-n{n}-x{copies}-{ids}", lay, 12, 4, 0.5, [(10, 14), (n - 3, n)], ("lds", "ws"), "classes",
                   class_of_chain=list(range(1, copies + 1)) + [1] * (n_chains - copies), same_place=same_place)
    if ids == "negative":
        case.class_ids = -(np.arange(n, dtype=np.int32)[::-1] + 1)
        case.closed = "all"
    elif ids == "none":
        case.class_ids, case.closed = None, None
    return case


def _nan32(negative):
    return float(np.array([0xFFC00000 if negative else 0x7FC00000], dtype=np.uint32).view(f32)[0])


@functools.lru_cache(maxsize=None)
def specials_case(n, kind):
    """n boxes in eight (12, 4) chains (heavy overlap). "equal": every score the same. "mixed": scores cycle through ties, NaN of
    both signs, +-inf, +-0 and denormals; three identical boxes; three identical zero-area boxes (0 / 0 is NaN: all three are
    kept); inverted boxes; a NaN coordinate in the box visited first and in the box visited last; infinite coordinates.
    No closed form: judged by nms_stepwise."""
    idx = np.arange(n)
    chain, k = idx % 8, idx // 8
    y, h = BAND * chain, 1 + chain % 17
    d = np.stack([y, k * 4, y + h - 1, k * 4 + 11, np.zeros(n)], 1).astype(f64)
    if kind == "equal":
        d[:, 4] = 0.25
        return Case(f"specials-n{n}-equal", d, 0.5, paths_for(n, True), group="specials")
    pool = [1.0, 0.5, 0.5, 0.25, _nan32(False), 2.0, float("inf"), 0.0, -0.0, 1e-40, -1e-40, 0.5, _nan32(True), float("-inf"),
            3.0, -1.0, 0.0, -0.0, 1.0]
    d[:, 4] = [pool[(i * 7) % len(pool)] for i in range(n)]
    d[20:23, :4] = d[20, :4]                                       # identical boxes
    d[30:33, :4] = (BAND * 9, 5, BAND * 9 + 3, 4)                  # x2 = x1 - 1: width 0, area 0
    d[40, :4] = (BAND * 10 + 9, 30, BAND * 10, 10)                 # inverted in both axes
    d[41, :4] = (BAND * 10, 10, BAND * 10 + 9, 30)
    d[0, 4], d[0, 1] = _nan32(False), float("nan")                 # visited first: the lowest index among the NaN scores
    d[n - 1, 4], d[n - 1, 2] = float("-inf"), float("nan")         # visited last: the highest index among the lowest scores
    d[50, 3], d[51, 0], d[52, :4] = float("inf"), float("-inf"), (float("-inf"), float("-inf"), float("inf"), float("inf"))
    order = visit_order(d)
    assert order[0] == 0 and order[-1] == n - 1
    return Case(f"specials-n{n}-mixed", d, 0.5, paths_for(n, True), group="specials")


@dataclasses.dataclass
class SegCase:
    name: str
    dets: np.ndarray            # float64 [S, n_max, 5]
    counts: np.ndarray          # int32 [S]
    parts: list                 # the Case of each segment's first counts[s] rows (None for an empty segment)
    thr: float = 0.5

    def expected(self):
        """keep [S, n_max] padded with -1, counts [S]."""
        s_, n_max = self.dets.shape[:2]
        keep, cnt = np.full((s_, n_max), -1, np.int64), np.zeros(s_, np.int32)
        for s, part in enumerate(self.parts):
            if part is not None:
                k = expected_keep(part)
                keep[s, :k.size], cnt[s] = k, k.size
        return keep, cnt


@functools.lru_cache(maxsize=None)
def segments_case(n_max):
    """S = 6 segments of n_max rows with counts n_max, 0, 1, 64, 65, n_max - 1: segment s holds composite(counts[s]) in its first
    rows; the rows behind hold NaN and +inf scores, NaN and infinite coordinates, and copies of the segment's own boxes under a
    higher score, which would suppress them if they were read."""
    counts = np.array([n_max, 0, 1, 64, 65, n_max - 1], np.int32)
    dets = np.zeros((6, n_max, 5), f64)
    parts = []
    for s, c in enumerate(counts):
        part = composite(int(c), 0.5) if c else None
        parts.append(part)
        if part is not None:
            dets[s, :c] = part.dets
        for r in range(c, n_max):
            real = dets[s, (r * 5) % c, :4] if c else np.zeros(4)
            dets[s, r] = [(*real, float("inf")), (*real, _nan32(r % 2 == 0)), (float("nan"), 0, 5, 5, 1e6),
                          (float("-inf"), float("-inf"), float("inf"), float("inf"), 1e6), (0, 0, 2.0 ** 19, 2.0 ** 19, float("inf")),
                          (*real, 1e6)][r % 6]
    return SegCase(f"segments-n{n_max}", dets, counts, parts)


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every single-segment case, by name."""
    out = []
    for n in COMPOSITE_SIZES:
        for thr in (0.5, 0.3, 0.7) if n in THREE_TYPE_SIZES else (0.5,):
            c = composite(n, thr)
            out.append(c)
            # every chain-neighbour pair sits exactly on thr: one float above it nothing is suppressed (`>=`, not `>`)
            out.append(with_threshold(c, next_up(thr), c.name + "-next-up", "all", "equality"))
    for n in (130, 1089):
        for copies in (2, 3):
            out += [classes_case(n, copies, ids) for ids in ("positive", "negative", "none")]
    for n in (70, 300):
        out += [specials_case(n, "equal"), specials_case(n, "mixed")]
    base = composite(130, 0.5, general=True)
    for thr, closed in ((0.0, "first"), (-1.0, "first"), (1.0, "all"), (1.5, "all"), (float("nan"), "all")):
        out.append(with_threshold(base, thr, f"threshold-n130-{thr}", closed, "threshold"))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return {c.name: c for c in out}
