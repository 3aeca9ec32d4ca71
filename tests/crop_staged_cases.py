"""The staged crop kernel (crop_forward_nchw_staged, csrc/crop.hip) restated on the host, and the launches that pin every regime
of its LDS-DMA ring. tests/test_crop_staged_host.py checks the restatement and the table without a GPU,
tests/test_gpu_crop_staged.py runs the launches (and, in a child process, the gather kernel on the same launches).

What is restated, each from the kernel's own lines:
  * footprint_slots     S = rows x 16-byte column segments of the samples inside the map (make_sample in fp32);
  * ring_geometry       BS, NB, G, K, D, ngroups, first_of, the last group's shift (`const int BS = ...` .. `ngroups`, first_of),
                        and for every group g the wait budget ahead * K + min(D, g) * G and the arm of the s_waitcnt vmcnt ladder
                        (cs_wait_vmcnt_at_most) it lands on;
  * div_by_reciprocal   cs_div_small and the slot -> (channel, row, segment) split: int((a + 0.5f) * rcp(b)) in fp32.

A launch's boxes are CONSTRUCTED (px_box: a box whose samples span exactly the given pixel rows and columns), so the footprint a
box names is the footprint the kernel computes; depth and num_boxes are picked so that the launcher (ops.crop_plan) chooses the
channels per wave the launch names. Which (G, K, D) and which ladder arms a launch reaches follows from that by ring_geometry;
coverage_problems() lists what the table fails to reach."""
import dataclasses
import functools

import numpy as np

RING_SLOTS = 512                                                        # CS_RING_SLOTS
LADDER = (32, 24, 20, 16, 14, 12, 10, 8, 7, 6, 5, 4, 3, 2, 1, 0)        # cs_wait_vmcnt_at_most's immediates, as tested
MAX_STAGED_SLOTS = 256                                                  # larger footprints: the in-launch gather fallback
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------------------------
def samples(c1, c2, size, crop):
    """make_sample (csrc/crop_math.hpp) for t = 0 .. crop - 1, in fp32, operation by operation: [(inside, lo, hi)]."""
    c1, c2 = f32(c1), f32(c2)
    out = []
    for t in range(crop):
        if crop > 1:
            scale = f32(f32(f32(c2 - c1) * f32(size - 1)) / f32(crop - 1))
            v = f32(f32(c1 * f32(size - 1)) + f32(f32(t) * scale))
        else:
            v = f32(0.5 * float(f32(c1 + c2)) * float(size - 1))
        inside = not (v < 0 or v > f32(size - 1))
        out.append((inside, int(np.floor(v)) if inside else 0, int(np.ceil(v)) if inside else 0))
    return out


def _crop_footprint_slots(box, size_h, size_w, ch, cw):
    """Host restatement of crop_forward_nchw_staged's footprint (csrc/crop.hip: make_sample in fp32, then S = rows x 16-byte
    column segments of the samples inside the map): None when no sample is inside, else S. S <= 256 takes the LDS-DMA path."""
    import numpy as np
    f = np.float32

    def samples(c1, c2, size, crop):
        c1, c2 = f(c1), f(c2)
        scale = f(f(f(c2 - c1) * f(size - 1)) / f(crop - 1))
        a = f(c1 * f(size - 1))
        out = []
        for t in range(crop):
            v = f(a + f(f(t) * scale))
            if not (v < 0 or v > f(size - 1)):
                out.append((int(np.floor(v)), int(np.ceil(v))))
        return out

    ys, xs = samples(box[0], box[2], size_h, ch), samples(box[1], box[3], size_w, cw)
    if not ys or not xs:
        return None
    ymin, ymax = min(lo for lo, _ in ys), max(hi for _, hi in ys)
    xmin, xmax = min(lo for lo, _ in xs), max(hi for _, hi in xs)
    return (ymax - ymin + 1) * (((xmax - (xmin & ~3)) >> 2) + 1)


def arm_of(budget):
    """The immediate cs_wait_vmcnt_at_most(budget) waits with: the largest of LADDER that does not exceed the budget."""
    return next(a for a in LADDER if budget >= a)


@dataclasses.dataclass(frozen=True)
class Ring:
    S: int
    nchan: int
    BS: int
    NB: int
    G: int
    K: int
    D: int
    ngroups: int
    budgets: tuple      # per group g: ahead * K + min(D, g) * G
    arms: tuple         # per group g: arm_of(budget)

    @property
    def gkd(self):
        return (self.G, self.K, self.D)


@functools.lru_cache(maxsize=None)
def ring_geometry(S, nchan, ring_slots=RING_SLOTS):
    """The ring of one (box, slab): a footprint of S <= 256 slots, nchan channels in the slab."""
    assert 1 <= S <= MAX_STAGED_SLOTS and nchan >= 1
    BS = 128 if S <= 128 else 256
    NB = ring_slots // BS
    G = min(8, BS // S, nchan)
    K = (G * S + 63) >> 6
    D = NB - 1
    ngroups = (nchan + G - 1) // G
    budgets = tuple(min(D, ngroups - 1 - g) * K + min(D, g) * G for g in range(ngroups))
    return Ring(S, nchan, BS, NB, G, K, D, ngroups, budgets, tuple(arm_of(b) for b in budgets))


def first_of(g, G, c_lo, depth):
    """The first channel group g's DMA moves: a group always moves G channels, so the last group of the image's last channels starts
    early enough to stay inside the image."""
    return min(c_lo + g * G, depth - G)


def last_shift(ring, c_lo, depth):
    """The channels the interpolation skips in front of the last group's buffer (c + shift): > 0 when the group's G channels would
    end past the image's last channel — a ragged last group of the last slab, or of the slab before a short last slab."""
    g = ring.ngroups - 1
    return c_lo + g * ring.G - first_of(g, ring.G, c_lo, depth)


def reachable(ring_slots=RING_SLOTS, cpws=(2, 4, 8, 16)):
    """Every (G, K, D), every ladder arm and the largest budget the kernel can meet with this ring: S in 1..256, nchan in
    1..cpw."""
    gkd, arms, top = set(), set(), 0
    for S in range(1, MAX_STAGED_SLOTS + 1):
        for nchan in range(1, max(cpws) + 1):
            r = ring_geometry(S, nchan, ring_slots)
            gkd.add(r.gkd)
            arms.update(r.arms)
            top = max(top, max(r.budgets))
    return gkd, arms, top


def rcp_candidates(b):
    """What v_rcp_f32 may return for the integer b: the correctly rounded fp32 reciprocal and its two neighbours (1 ulp)."""
    r = (f32(1.0) / np.asarray(b, dtype=f32)).astype(f32)
    return np.nextafter(r, f32(0)), r, np.nextafter(r, f32(np.inf))


def div_by_reciprocal(a, r):
    """int((float(a) + 0.5f) * r) in fp32: the kernel's quotient of a by b given r ~ 1 / b."""
    return ((np.asarray(a, dtype=f32) + f32(0.5)) * np.asarray(r, dtype=f32)).astype(f32).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# constructed boxes
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Box:
    kind: str           # "ring": constructed, S named; "fallback": S named, > 256; "partly": S computed by the restatement;
    #                     "outside": no sample inside the map; "corner": the single point (H - 1, W - 1), S = 1
    coords: tuple       # normalised (y1, x1, y2, x2)
    S: object           # the footprint the box names (None: no sample inside)
    bad_index: int = 0  # != 0: the box_index this box is given instead of a valid one


def _edge(lo_px, n_px, size):
    """Normalised (c1, c2) whose samples span exactly the pixels lo_px .. lo_px + n_px - 1 of a map side of `size` pixels: from a
    quarter pixel inside the first to a quarter pixel inside the last (n_px >= 2), or the pixel itself (n_px == 1; only pixels
    whose coordinate survives the division and the multiplication in fp32 are asked for)."""
    assert 0 <= lo_px and lo_px + n_px <= size and n_px >= 1
    if n_px == 1:
        c = f32(lo_px) / f32(size - 1)
        assert f32(c * f32(size - 1)) == f32(lo_px), (lo_px, size)
        return float(c), float(c)
    return (lo_px + 0.25) / (size - 1), (lo_px + n_px - 1.25) / (size - 1)


def px_box(h, w, r0, rows, c0, cols, reverse=False):
    """The box whose samples (any crop size >= 2 x 2) touch exactly the map rows r0 .. r0 + rows - 1 and columns c0 .. c0 + cols - 1,
    and the footprint that makes: rows x the 16-byte segments from c0 & ~3 to the last column."""
    y1, y2 = _edge(r0, rows, h)
    x1, x2 = _edge(c0, cols, w)
    if reverse:     # samples run from the far edge back: the same pixels
        y1, y2, x1, x2 = y2, y1, x2, x1
    return (y1, x1, y2, x2), rows * (((c0 + cols - 1 - (c0 & ~3)) >> 2) + 1)


# footprints as (rows, segments): every S class of the ring — the borders of G = BS / S (8 | 9, 9 | 10, 10 | 11, 12 | 13, 16 | 17,
# 18, 21 | 22, 25 | 26, 32 | 33, 42 | 44, 64 | 65), of K (G * S across 64), of BS (128 | 130) and of the ring (256)
FOOTPRINTS = ((1, 1), (2, 2), (2, 4), (8, 1), (3, 3), (9, 1), (5, 2), (11, 1), (3, 4), (13, 1), (4, 4), (17, 1), (6, 3), (7, 3),
              (11, 2), (5, 5), (13, 2), (8, 4), (11, 3), (7, 6), (11, 4), (8, 8), (13, 5), (16, 8), (26, 5), (24, 8), (28, 7),
              (32, 8))


@dataclasses.dataclass(frozen=True)
class Launch:
    name: str
    batch: int
    depth: int
    h: int
    w: int
    num_boxes: int
    ch: int
    cw: int
    cpw: int            # what ops.crop_plan must answer
    map_mode: int

    @property
    def id(self):
        return self.name

    @property
    def plane(self):
        return self.ch * self.cw

    @property
    def slabs(self):
        return -(-self.depth // self.cpw)

    def nchans(self):
        """Channels of every slab."""
        return [min(self.depth, (s + 1) * self.cpw) - s * self.cpw for s in range(self.slabs)]


EXTRAPOLATION = -1.25

LAUNCHES = (
    # cpw 16 needs num_boxes * slabs >= 4096. Slabs of 16 and 15 channels: arms 10, 12, 14 and every K = 2 combination
    Launch("cpw16-d31-48x32-2x2", 2, 31, 48, 32, 2048, 2, 2, 16, 2),
    # cpw 8: slabs of 8 and 7 / 5 / 6 channels (G = nchan = 5, 6, 7 with K = 1 exist nowhere else)
    Launch("cpw8-d15-64x64-4x4", 2, 15, 64, 64, 2048, 4, 4, 8, 2),
    Launch("cpw8-d13-40x48-2x2", 1, 13, 40, 48, 2048, 2, 2, 8, 2),
    Launch("cpw8-d14-64x64-7x8", 2, 14, 64, 64, 2048, 7, 8, 8, 2),            # plane 56: 14 active lanes
    Launch("cpw4-d7-64x64-2x4", 2, 7, 64, 64, 2048, 2, 4, 4, 2),              # slabs of 4 and 3 channels
    Launch("cpw2-d5-64x64-2x2-grid", 3, 5, 64, 64, 37, 2, 2, 2, 0),           # 3 slabs: the plain (box, slab) grid; nchan 2, 2, 1
    Launch("cpw2-d15-64x64-3x4-xcd", 2, 15, 64, 64, 50, 3, 4, 2, 1),          # 8 slabs: map mode 1
    Launch("cpw2-d3-64x64-4x4-ragged", 2, 3, 64, 64, 41, 4, 4, 2, 2),         # 2 slabs on 4 XCDs each, 41 boxes: the last round is short
    # the H * W >= 65536 rule: 8 channels per wave where a smaller map would get 16; one slab on all 8 XCDs, 4100 = 8 * 512 + 4
    Launch("cpw8-d8-256x256-2x2", 1, 8, 256, 256, 4100, 2, 2, 8, 2),
    Launch("cpw8-d31-64x64-14x14", 2, 31, 64, 64, 1024, 14, 14, 8, 2),        # plane 196: 49 active lanes
    # plane 256: every lane active; the fallback's tap table (8704 B) is larger than the ring. 16 slabs: map mode 1
    Launch("cpw2-d32-64x64-16x16", 2, 32, 64, 64, 128, 16, 16, 2, 1),
)


@functools.lru_cache(maxsize=None)
def boxes_of(launch):
    """The launch's boxes, in order: the menu (every footprint of FOOTPRINTS that fits the map, then the special boxes) over and
    over, each visit at another place of the map — the first at the top left, the second against the bottom right edge."""
    h, w = launch.h, launch.w
    menu = [fp for fp in FOOTPRINTS if fp[0] <= h and 4 * fp[1] <= w]
    specials = ("fallback", "outside", "partly", "corner", "bad_high", "bad_negative")
    period = len(menu) + len(specials)
    out = []
    for i in range(launch.num_boxes):
        visit, j = divmod(i, period)
        v = visit % 8
        if j < len(menu):
            rows, segs = menu[j]
            off = v % 4                               # the first column's place inside its 16-byte segment
            cols = 4 * segs - off - (v >> 2 & 1)
            if cols < 2:
                off, cols = 0, 4 * segs
            r_free, s_free = h - rows, w // 4 - segs
            r0 = 0 if v == 0 else r_free if v == 1 else (v * 7) % (r_free + 1)
            s0 = 0 if v == 0 else s_free if v == 1 else (v * 5) % (s_free + 1)
            if rows == 1:                              # a pixel row of its own: 0 and H - 1 are exact in fp32
                r0 = 0 if v % 2 == 0 else h - 1
            coords, S = px_box(h, w, r0, rows, 4 * s0 + off, cols, reverse=v % 3 == 2)
            out.append(Box("ring" if S <= MAX_STAGED_SLOTS else "fallback", coords, S))
            continue
        kind = specials[j - len(menu)]
        if kind == "fallback":                         # the whole map
            out.append(Box(kind, (0.0, 0.0, 1.0, 1.0), h * (w // 4)))
        elif kind == "outside":
            out.append(Box(kind, (-0.5, -0.5, -0.1, -0.1), None))
        elif kind == "partly":                         # over the top and the left edge (v even) / the bottom and the right one
            c = (-0.2, -0.05, 0.12, 0.2) if v % 2 == 0 else (0.9, 0.85, 1.15, 1.04)
            out.append(Box(kind, c, _crop_footprint_slots(c, h, w, launch.ch, launch.cw)))
        elif kind == "corner":                         # every sample ON the map's last pixel: the pair read's second dword is
            out.append(Box(kind, (1.0, 1.0, 1.0, 1.0), 1))   # the one past the footprint's last slot
        else:
            coords, S = px_box(h, w, 3, 4, 8, 7)
            out.append(Box("ring", coords, S, bad_index=launch.batch + 3 if kind == "bad_high" else -1))
    return tuple(out)


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31)


def build(launch):
    """image [B,C,H,W] fp32 (standard normal, every |v| < 0.05 replaced by -0.0), boxes [N,4] fp32, index int32 [N] as the kernel
    gets it, valid_index (the bad ones replaced by 0: what the oracle is asked), bad [N] bool."""
    rng = np.random.Generator(np.random.PCG64(_seed(launch.name)))
    image = rng.standard_normal((launch.batch, launch.depth, launch.h, launch.w), dtype=np.float32)
    image[np.abs(image) < 0.05] = -0.0
    bx = boxes_of(launch)
    boxes = np.array([b.coords for b in bx], dtype=np.float32)
    valid = (np.arange(len(bx)) % launch.batch).astype(np.int32)
    bad = np.array([b.bad_index != 0 for b in bx])
    index = np.where(bad, np.array([b.bad_index for b in bx]), valid).astype(np.int32)
    valid[bad] = 0
    return dict(image=image, boxes=boxes, index=index, valid_index=valid, bad=bad)


# ---------------------------------------------------------------------------------------------------------------------
# what the table reaches
# ---------------------------------------------------------------------------------------------------------------------
def rings_of(launch):
    """[(box, slab, Ring, shift of the last group)] of every (box, slab) of the launch that goes through the ring: a constructed
    footprint of at most 256 slots and a valid box_index."""
    out = []
    nchans = launch.nchans()
    for b in boxes_of(launch):
        if b.kind not in ("ring", "corner") or b.bad_index:
            continue
        for s, nchan in enumerate(nchans):
            r = ring_geometry(b.S, nchan)
            out.append((b, s, r, last_shift(r, s * launch.cpw, launch.depth)))
    return out


def on_pixel_samples(launch):
    """Does a ring box of the launch have a column sample ON a pixel (X.hi == X.lo)?"""
    return any(any(ins and lo == hi for ins, lo, hi in samples(b.coords[1], b.coords[3], launch.w, launch.cw))
               for b in boxes_of(launch) if b.kind in ("ring", "corner") and not b.bad_index)


def reached(launches=LAUNCHES):
    """(the (G, K, D) set, the ladder arms) the launches' constructed boxes reach."""
    gkd, arms = set(), set()
    for launch in launches:
        for _, _, r, _ in rings_of(launch):
            gkd.add(r.gkd)
            arms.update(r.arms)
    return gkd, arms


def coverage_problems(launches=LAUNCHES):
    """What the table lacks of the regimes it promises ([] = nothing)."""
    out = []
    want_gkd, want_arms, _ = reachable()
    rings = [(launch, *t) for launch in launches for t in rings_of(launch)]
    gkd, arms = reached(launches)
    out += [f"missing: ladder arm {a}" for a in sorted(want_arms - arms)]
    out += [f"missing: (G, K, D) = {c}" for c in sorted(want_gkd - gkd)]
    checks = {
        "ngroups < D": lambda l, b, s, r, sh: r.ngroups < r.D,
        "ngroups == D": lambda l, b, s, r, sh: r.ngroups == r.D,
        "ngroups >= D + 2": lambda l, b, s, r, sh: r.ngroups >= r.D + 2,
        "ngroups >= D + 2 in a 256-slot buffer (D = 1)": lambda l, b, s, r, sh: r.D == 1 and r.ngroups >= 3,
        "a ragged last group with shift > 0 at the end of the image's channels": lambda l, b, s, r, sh: sh > 0 and s == l.slabs - 1,
        "shift > 0 in the slab before a short last slab": lambda l, b, s, r, sh: sh > 0 and s < l.slabs - 1,
        "a ragged last group inside the image (shift 0, fewer than G channels wanted)":
            lambda l, b, s, r, sh: sh == 0 and r.nchan % r.G != 0,
        "a last slab with nchan < cpw": lambda l, b, s, r, sh: s == l.slabs - 1 and r.nchan < l.cpw,
        "BS 128": lambda l, b, s, r, sh: r.BS == 128,
        "BS 256": lambda l, b, s, r, sh: r.BS == 256,
    }
    checks.update({f"K = {k}": (lambda l, b, s, r, sh, k=k: r.K == k) for k in (1, 2, 3, 4)})
    for what, ok in checks.items():
        if not any(ok(*t) for t in rings):
            out.append("missing: " + what)
    for cpw in (2, 4, 8, 16):
        if not any(l.cpw == cpw for l in launches):
            out.append(f"missing: cpw {cpw}")
    for mode in (0, 1, 2):
        if not any(l.map_mode == mode for l in launches):
            out.append(f"missing: map mode {mode}")
    if not any(l.map_mode == 2 and l.num_boxes % (8 // l.slabs) for l in launches):
        out.append("missing: map mode 2 with num_boxes no multiple of 8 / slabs")
    for plane in (4, 56, 196, 256):
        if not any(l.plane == plane for l in launches):
            out.append(f"missing: plane {plane}")
    if not any(l.h * l.w >= 65536 and l.cpw == 8 and l.num_boxes * -(-l.depth // 16) >= 4096 for l in launches):
        out.append("missing: the H * W >= 65536 rule where a smaller map would get 16 channels per wave")
    # beside ring boxes, in ONE launch: the gather fallback, a box wholly outside, a bad box_index, a box partly outside, samples on
    # pixels (negative zeros are in every image: build())
    def mixed(l):
        bx = boxes_of(l)
        kinds = {b.kind for b in bx}
        partly = [b for b in bx if b.kind == "partly"]
        return ({"ring", "fallback", "outside", "partly"} <= kinds and any(b.bad_index > 0 for b in bx) and
                any(b.bad_index < 0 for b in bx) and all(b.S is not None and b.S <= MAX_STAGED_SLOTS for b in partly) and
                on_pixel_samples(l))
    if not any(mixed(l) for l in launches):
        out.append("missing: a launch with the fallback, an outside box, bad indices, a partly outside ring box and on-pixel samples")
    for l in launches:
        if l.num_boxes * l.depth * l.plane > 15_000_000:
            out.append(f"{l.name}: more than 15 M output elements")
        if (l.h > 64 or l.w > 64) and (l.h, l.w, l.depth) != (256, 256, 8):
            out.append(f"{l.name}: a map larger than 64 x 64")
    return out
