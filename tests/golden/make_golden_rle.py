#!/usr/bin/env python3
"""Regenerates tests/golden/rle.npz from the reference's own RLE codec.

    python tests/golden/make_golden_rle.py          (reference tree: $MASKRCNN_REFERENCE, as for make_golden.py)

Compiles <reference>/cocoapi/common/maskApi.c into a temporary directory OUTSIDE this repository (nothing of it is kept),
calls rleEncode, rleToString, rleArea and rleToBbox through ctypes on the cases below and stores DATA only:
    names                      case names
    shapes   int32 [K,2]       (h, w)
    bits     uint8             np.packbits of every row-major mask, concatenated;  bit_off int64 [K+1]
    counts   uint32            run lengths, concatenated;                          cnt_off int64 [K+1]
    strings  uint8             compressed strings, concatenated;                   str_off int64 [K+1]
    areas    int32 [K],  bboxes int32 [K,4] (x, y, w, h)
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class RLE(ctypes.Structure):   # typedef struct { siz h, w, m; uint *cnts; } RLE;  siz = unsigned long
    _fields_ = [("h", ctypes.c_ulong), ("w", ctypes.c_ulong), ("m", ctypes.c_ulong), ("cnts", ctypes.POINTER(ctypes.c_uint))]


def load_codec(reference: str, tmp: str) -> ctypes.CDLL:
    src = os.path.join(reference, "cocoapi", "common", "maskApi.c")
    lib = os.path.join(tmp, "libmaskapi.so")
    subprocess.run(["cc", "-O2", "-std=c99", "-shared", "-fPIC", "-I" + os.path.dirname(src), src, "-lm", "-o", lib], check=True)
    dll = ctypes.CDLL(lib)
    dll.rleEncode.argtypes = [ctypes.POINTER(RLE), ctypes.c_void_p, ctypes.c_ulong, ctypes.c_ulong, ctypes.c_ulong]
    dll.rleEncode.restype = None
    dll.rleToString.argtypes = [ctypes.POINTER(RLE)]
    dll.rleToString.restype = ctypes.c_void_p          # malloc'ed char*: copied, then freed
    dll.rleArea.argtypes = [ctypes.POINTER(RLE), ctypes.c_ulong, ctypes.POINTER(ctypes.c_uint)]
    dll.rleToBbox.argtypes = [ctypes.POINTER(RLE), ctypes.POINTER(ctypes.c_double), ctypes.c_ulong]
    dll.rleFree.argtypes = [ctypes.POINTER(RLE)]
    return dll


def encode(dll, mask: np.ndarray):
    h, w = mask.shape
    col_major = np.asfortranarray(mask.astype(np.uint8))        # maskUtils.encode's input layout
    r = RLE()
    dll.rleEncode(ctypes.byref(r), col_major.ctypes.data, h, w, 1)
    counts = np.array([r.cnts[i] for i in range(r.m)], dtype=np.uint32)
    sp = dll.rleToString(ctypes.byref(r))
    string = np.frombuffer(ctypes.string_at(sp), dtype=np.uint8).copy()
    ctypes.CDLL(None).free(ctypes.c_void_p(sp))
    area = ctypes.c_uint()
    dll.rleArea(ctypes.byref(r), 1, ctypes.byref(area))
    bb = (ctypes.c_double * 4)()
    dll.rleToBbox(ctypes.byref(r), bb, 1)
    dll.rleFree(ctypes.byref(r))
    return counts, string, int(area.value), [int(v) for v in bb]


def cases():
    rng = np.random.default_rng(20240917)
    out = []
    for i, (h, w, d) in enumerate([(5, 7, 0.5), (16, 16, 0.1), (37, 53, 0.5), (64, 61, 0.9), (33, 130, 0.02), (128, 95, 0.3),
                                   (9, 1023, 0.5), (200, 7, 0.7), (71, 66, 0.5), (50, 50, 0.001), (3, 3, 0.5), (97, 101, 0.25)]):
        out.append((f"random{i}_{h}x{w}_d{d}", rng.random((h, w)) < d))
    out.append(("empty_40x30", np.zeros((40, 30), bool)))
    out.append(("empty_1x1", np.zeros((1, 1), bool)))
    out.append(("full_40x30", np.ones((40, 30), bool)))
    out.append(("full_1x1", np.ones((1, 1), bool)))
    out.append(("full_17x5", np.ones((17, 5), bool)))
    out.append(("row_1x77", rng.random((1, 77)) < 0.5))
    out.append(("row_1x4_on", np.ones((1, 4), bool)))
    out.append(("col_91x1", rng.random((91, 1)) < 0.5))
    out.append(("col_64x1_on", np.ones((64, 1), bool)))
    yy, xx = np.mgrid[0:64, 0:64]
    out.append(("checker_64x64", (yy + xx) % 2 == 1))
    out.append(("checker_on_first_33x35", (np.mgrid[0:33, 0:35].sum(0)) % 2 == 0))
    m = np.zeros((20, 21), bool); m[0, 0] = True
    out.append(("first_pixel_only_20x21", m))
    m = rng.random((45, 46)) < 0.4; m[0, 0] = True
    out.append(("first_pixel_on_45x46", m))
    m = np.zeros((24, 10), bool); m[20:, 3] = True; m[:5, 4] = True       # bottom of column 3 into the top of column 4
    out.append(("wrap_24x10", m))
    m = np.zeros((32, 9), bool); m[31, :] = True; m[0, :] = True            # every column's end joins the next one's start
    out.append(("wrap_every_column_32x9", m))
    m = np.zeros((40, 6), bool); m[35:, 2] = True; m[:, 3] = True; m[:7, 4] = True   # a run across a whole column
    out.append(("wrap_through_column_40x6", m))
    m = np.zeros((16, 8), bool); m[8:, 7] = True                            # on up to the last pixel
    out.append(("last_pixel_on_16x8", m))
    for w in (1, 2, 3, 5, 6, 7, 13, 1021):
        out.append((f"width{w}_29x{w}", rng.random((29, w)) < 0.5))
    m = np.zeros((60, 90), bool); m[10:40, 20:75] = True
    out.append(("rect_60x90", m))
    m = np.zeros((60, 90), bool); m[10:40, 20:75] = True
    out.append(("noisy_rect_60x90", m ^ (rng.random((60, 90)) < 0.03)))
    m = np.zeros((70, 40), bool); m[0:70, 0:12] = True; m[30:50, 30:40] = True
    out.append(("two_rects_touching_edges_70x40", m))
    yy, xx = np.mgrid[0:300, 0:420]
    out.append(("ellipse_300x420", ((yy - 140) / 110.0) ** 2 + ((xx - 230) / 170.0) ** 2 <= 1.0))
    yy, xx = np.mgrid[0:360, 0:250]
    ang = np.arctan2(yy - 180, xx - 120)
    rad = 80 + 25 * np.sin(3 * ang) + 12 * np.cos(7 * ang)
    out.append(("blob_360x250", np.hypot(yy - 180, xx - 120) <= rad))
    return out


def main():
    reference = os.environ.get("MASKRCNN_REFERENCE", "/root/reference")
    with tempfile.TemporaryDirectory() as tmp:
        dll = load_codec(reference, tmp)
        names, shapes, bits, counts, strings, areas, bboxes = [], [], [], [], [], [], []
        for name, mask in cases():
            c, s, a, bb = encode(dll, mask)
            names.append(name); shapes.append(mask.shape); bits.append(np.packbits(mask.reshape(-1)))
            counts.append(c); strings.append(s); areas.append(a); bboxes.append(bb)
    off = lambda parts: np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    path = os.path.join(HERE, "rle.npz")
    np.savez_compressed(path, names=np.array(names), shapes=np.array(shapes, np.int32),
                        bits=np.concatenate(bits), bit_off=off(bits), counts=np.concatenate(counts), cnt_off=off(counts),
                        strings=np.concatenate(strings), str_off=off(strings), areas=np.array(areas, np.int32),
                        bboxes=np.array(bboxes, np.int32))
    print(f"{path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
