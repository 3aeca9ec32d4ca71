#!/usr/bin/env python3
"""Regenerates tests/golden/codec.npz from the reference's own RLE codec.

    python tests/golden/make_golden_codec.py        (reference tree: $MASKRCNN_REFERENCE, as for make_golden_rle.py)

Compiles <reference>/cocoapi/common/maskApi.c into a temporary directory OUTSIDE this repository (nothing of it is kept), calls
rleToString, rleFrString, rleArea, rleToBbox and rleDecode through ctypes on the run lists below and stores DATA only:
    names                      case names
    shapes   int32 [K,2]       (h, w) handed to the codec
    counts   uint32            run lengths, concatenated;                 cnt_off int64 [K+1]
    strings  uint8             rleToString of the counts, concatenated;   str_off int64 [K+1]
    fr_equal bool [K]          rleFrString(string) returned the counts (always true; stored as the generator's own check)
    areas    int32 [K],  bboxes int32 [K,4] (x, y, w, h)
    has_bits bool [K]          the runs cover exactly h*w pixels and the mask is small: rleDecode's output is stored
    bits     uint8             np.packbits of the ROW-major mask (rleDecode writes column-major; transposed here);  bit_off int64 [K+1]
Every string is a valid input for the reference: bytes 48..111, no token longer than 6 characters.
"""
import ctypes
import os
import tempfile

import numpy as np

from make_golden_rle import RLE, load_codec

HERE = os.path.dirname(os.path.abspath(__file__))


def bind(dll):
    dll.rleFrString.argtypes = [ctypes.POINTER(RLE), ctypes.c_char_p, ctypes.c_ulong, ctypes.c_ulong]
    dll.rleFrString.restype = None
    dll.rleDecode.argtypes = [ctypes.POINTER(RLE), ctypes.c_void_p, ctypes.c_ulong]
    dll.rleDecode.restype = None
    dll.rleInit.argtypes = [ctypes.POINTER(RLE), ctypes.c_ulong, ctypes.c_ulong, ctypes.c_ulong, ctypes.POINTER(ctypes.c_uint)]
    dll.rleInit.restype = None
    return dll


def run_case(dll, counts, h, w, want_bits):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    r = RLE()
    dll.rleInit(ctypes.byref(r), h, w, counts.size, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)))
    sp = dll.rleToString(ctypes.byref(r))
    string = ctypes.string_at(sp)
    ctypes.CDLL(None).free(ctypes.c_void_p(sp))
    area = ctypes.c_uint()
    dll.rleArea(ctypes.byref(r), 1, ctypes.byref(area))
    bb = (ctypes.c_double * 4)()
    dll.rleToBbox(ctypes.byref(r), bb, 1)
    bits = np.zeros(0, np.uint8)
    if want_bits:
        col_major = np.empty(h * w, dtype=np.uint8)
        dll.rleDecode(ctypes.byref(r), col_major.ctypes.data, 1)
        bits = np.packbits(col_major.reshape(w, h).T.reshape(-1))
    back = RLE()
    dll.rleFrString(ctypes.byref(back), string, h, w)
    got = np.array([back.cnts[i] for i in range(back.m)], dtype=np.uint32)
    dll.rleFree(ctypes.byref(back))
    dll.rleFree(ctypes.byref(r))
    s = np.frombuffer(string, dtype=np.uint8).copy()
    assert ((s >= 48) & (s <= 111)).all()
    return s, bool(np.array_equal(got, counts)), np.int32(np.uint32(area.value)), [int(v) for v in bb], bits


def mask_counts(mask):
    flat = np.concatenate([[0], np.asfortranarray(mask).reshape(-1, order="F").astype(np.int8)])
    edges = np.nonzero(np.diff(flat))[0]
    return np.diff(np.concatenate([[0], edges, [mask.size]])).astype(np.uint32)


def counts_with_string_length(rng, length):
    """A run list whose string has exactly `length` characters and no token boundary at a multiple of 64 (so a multi-character
    token straddles every one). Token lengths 1..4 are drawn; a difference x needs k characters when it lies in
    [-2^(5k-1), 2^(5k-1)) and not in [-2^(5k-6), 2^(5k-6)); the signs keep every run in [1, 2^27)."""
    lens, pos = [], 0
    while pos < length:
        ok = [k for k in (1, 2, 3, 4) if pos + k <= length and ((pos + k) % 64 != 0 or pos + k == length)]
        lens.append(int(rng.choice(ok)))
        pos += lens[-1]
    cnts = []
    for m, k in enumerate(lens):
        mag = int(rng.integers(0 if k == 1 else 1 << (5 * k - 6), 1 << (5 * k - 1)))
        prev = cnts[m - 2] if m > 2 else 0
        if prev - mag - 1 >= 1 and (rng.random() < 0.5 or prev + mag >= (1 << 27)):
            x = -mag - 1
        else:
            x = mag if prev + mag >= 1 or m == 0 else 1
        cnts.append(prev + x)
    return np.array(cnts, dtype=np.uint32)


def cases():
    rng = np.random.default_rng(20250214)
    out = []   # (name, counts, h, w)
    col = lambda name, c: out.append((name, np.array(c, dtype=np.uint32), int(np.sum(c, dtype=np.int64)) or 1, 1))
    for k in range(6):                                      # around the m > 2 rule
        col(f"tokens{k}", [3, 4, 5, 6, 7][:k])
    for d in (15, 16, -16, -17):                            # the sign boundary of a one-character difference
        col(f"diff{d}", [7, 40, 9, 40 + d, 5])
    for k in range(1, 7):                                   # tokens of every length, positive and negative
        c = [1, 1, (1 << (5 * k - 2)) - 4, 1, 1]
        if k >= 4:                                          # 2^18, 2^23, 2^28 pixels: a side stays within 16384
            out.append((f"toklen{k}", np.array(c, np.uint32), 1 << (5 * k - 2) // 2, 1 << (5 * k - 1) // 2))
        else:
            col(f"toklen{k}", [1, 1, 1 << (5 * k - 2), 1, 1])
    for length in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        c = counts_with_string_length(rng, length)
        out.append((f"chars{length}", c, 1, 1))            # a string test: the size does not fit the runs
    for k in (63, 64, 65, 1023, 1024, 1025):               # row lengths around the wave and its multiples
        c = rng.integers(1, 16, size=k).astype(np.int64)
        c[-1] += (-int(c.sum())) % 37
        out.append((f"runs{k}_37", c.astype(np.uint32), 37, int(c.sum()) // 37))
    out.append(("empty_5x7", np.array([35], np.uint32), 5, 7))
    out.append(("full_5x7", np.array([0, 35], np.uint32), 5, 7))
    for name, (y, x) in (("tl", (0, 0)), ("bl", (5, 0)), ("tr", (0, 4)), ("br", (5, 4))):
        m = np.zeros((6, 5), bool); m[y, x] = True
        out.append((f"corner_{name}_6x5", mask_counts(m), 6, 5))
    m = np.zeros((24, 10), bool); m[20:, 3] = True; m[:5, 4] = True        # an on run from column 3 into column 4
    out.append(("cross_column_24x10", mask_counts(m), 24, 10))
    out.append(("row_1x9", mask_counts(rng.random((1, 9)) < .5), 1, 9))
    out.append(("col_9x1", mask_counts(rng.random((9, 1)) < .5), 9, 1))
    out.append(("one_run_16384sq", np.array([0, 1 << 28], np.uint32), 16384, 16384))
    out.append(("mixed_a_13x17", mask_counts(rng.random((13, 17)) < .4), 13, 17))
    out.append(("mixed_b_40x9", mask_counts(rng.random((40, 9)) < .6), 40, 9))
    for h, w in ((1, 1), (1, 9), (9, 1), (5, 7), (37, 53), (64, 61), (65, 64), (33, 130)):   # decode: tile and edge sizes
        out.append((f"decode_{h}x{w}", mask_counts(rng.random((h, w)) < .5), h, w))
        m = rng.random((h, w)) < .3; m[0, 0] = True; m[-1, -1] = False
        out.append((f"decode_leading_zero_odd_{h}x{w}", mask_counts(m), h, w))
        out.append((f"decode_empty_{h}x{w}", np.array([h * w], np.uint32), h, w))
        out.append((f"decode_full_{h}x{w}", np.array([0, h * w], np.uint32), h, w))
    return out


def main():
    reference = os.environ.get("MASKRCNN_REFERENCE", "/root/reference")
    names, shapes, counts, strings, fr, areas, bboxes, has_bits, bits = [], [], [], [], [], [], [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        dll = bind(load_codec(reference, tmp))
        for name, c, h, w in cases():
            want = int(c.astype(np.int64).sum()) == h * w and h * w <= (1 << 20)
            s, same, a, bb, b = run_case(dll, c, h, w, want)
            assert same, name
            if name.startswith("chars"):
                assert s.size == int(name[5:]), (name, s.size)
            names.append(name); shapes.append((h, w)); counts.append(c); strings.append(s); fr.append(same)
            areas.append(a); bboxes.append(bb); has_bits.append(want); bits.append(b)
    off = lambda parts: np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    path = os.path.join(HERE, "codec.npz")
    np.savez_compressed(path, names=np.array(names), shapes=np.array(shapes, np.int32), counts=np.concatenate(counts),
                        cnt_off=off(counts), strings=np.concatenate(strings), str_off=off(strings), fr_equal=np.array(fr),
                        areas=np.array(areas, np.int32), bboxes=np.array(bboxes, np.int32), has_bits=np.array(has_bits),
                        bits=np.concatenate(bits), bit_off=off(bits))
    print(f"{path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
