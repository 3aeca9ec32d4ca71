#!/usr/bin/env python3
"""Regenerates tests/golden/roi_align_backward.npz from the reference's own code.

    python tests/golden/make_golden_roi_align_backward.py      (reference tree: $MASKRCNN_REFERENCE, as for make_golden.py)

The reference's roi_align (model.py:276-393) is differentiable through CropFunction.backward -> crop_backward, level by level.
CropFunction is a legacy autograd Function (c++ext/maskrcnn/__init__.py:25-45), which no longer runs under this torch, so the
script cannot call .backward(); it asks the reference for the two things that backward is made of:
  * the level of every box: the unmodified model.roi_align on four constant-valued maps (level l holds the value l) at pool size 1
    returns, for a box whose centre lies inside the image, the constant of the map it was cropped from (make_golden.gen_roi_levels
    reads levels the same way);
  * per level, the reference extension's crop_backward (crop_cpu.cpp:167-265) on that level's boxes in ascending box index — the
    order roi_align hands them to CropFunction — and on their rows of the incoming gradient.
The backward of roi_align's `cat` and inverse permutation only routes row r of the gradient to box r, which is what taking those
rows does.

Checked here on the CPU before anything is stored: every box's centre is inside the image, its unrounded level is at least 1e-3
away from 2.5, 3.5 and 4.5 (so no log2 implementation can disagree with torch's about a level), all four levels occur, and the
boxes include ones that spill outside [0, 1], ones whose samples sit on grid lines (lerp == 0), a zero-area box and several piled
on one object.

DATA only: image_shape, map_sizes [4,2], rois float32 [R,4], levels int32 [R], and per pool p in (7, 14, 1): grad_out_p<p> float32
[R,p,p,C] (NHWC; C = 8, and 4 at pool 14, which keeps the file small, as do values on a grid of eighths — the lerp weights are on no
grid, so every term still rounds) and g<l>_p<p> float32 [1,H_l,W_l,C] (NHWC) for l = 0..3.
"""
import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import roi_align_backward_cases as rc  # noqa: E402

IMAGE_SHAPE = (128, 128, 3)
MAP_SIZES = [(32, 32), (16, 16), (8, 8), (4, 4)]
CHANNELS = {7: 8, 14: 4, 1: 8}
POOLS = (7, 14, 1)


def reference_levels(rmodel, rois):
    """The level model.roi_align gives every box, read off its own output: one channel, pool 1, map l filled with l."""
    assert bool(((rois[:, 0] + rois[:, 2] >= 0) & (rois[:, 0] + rois[:, 2] <= 2) & (rois[:, 1] + rois[:, 3] >= 0) &
                 (rois[:, 1] + rois[:, 3] <= 2)).all()), "a box whose centre is outside the image would read 0, not its level"
    maps = [torch.full((1, 1, h, w), float(level)) for level, (h, w) in zip((2, 3, 4, 5), MAP_SIZES)]
    pooled = rmodel.roi_align([torch.from_numpy(rois).unsqueeze(0)] + maps, 1, np.array(IMAGE_SHAPE)).reshape(-1).numpy()
    assert len(pooled) == len(rois) and set(pooled.tolist()) <= {2.0, 3.0, 4.0, 5.0}, sorted(set(pooled.tolist()))
    return pooled.astype(np.int32)


def reference_backward(refc, rois, levels, grad_nchw):
    """The reference extension's crop_backward, once per level, on the boxes of that level in ascending index → [1,C,H_l,W_l] each."""
    out = []
    for level, (h, w) in zip((2, 3, 4, 5), MAP_SIZES):
        rows = np.flatnonzero(levels == level)
        gi = torch.zeros(1, grad_nchw.size(1), h, w)
        if len(rows):
            refc.crop_backward(grad_nchw[rows].contiguous(), torch.from_numpy(rois[rows]).contiguous(),
                               torch.zeros(len(rows), dtype=torch.int32), gi)
        out.append(gi)
    return out


def make_rois():
    rng = np.random.default_rng(20240607)
    area = float(IMAGE_SHAPE[0] * IMAGE_SHAPE[1])
    parts = [rc.boxes_on(rng, n, level, area) for level, n in ((2, 12), (3, 8), (4, 5), (5, 3))]
    s2 = 12.0 / 31.0
    fixed = np.array([
        [0.0, 0.0, 1.0, 1.0],                       # level 3 (16 x 16): pool 7 samples 0, 2.5, 5, ..: lerp == 0 on every other one
        [0.0, 0.0, s2, s2],                         # level 2 (32 x 32): pool 7 samples 0, 2, 4, ..: all on grid lines
        [-0.3, -0.2, 0.4, 0.5],                     # spills over the top left corner
        [0.6, 0.7, 1.3, 1.25],                      # spills over the bottom right corner (its centre stays inside: reference_levels)
        [-1.0, -1.0, 2.0, 2.0],                     # level 5, mostly outside
        [0.4, 0.3, 0.4, 0.3],                       # zero area (level 2: the reference's int cast of -inf)
        [0.30, 0.30, 0.62, 0.58], [0.31, 0.29, 0.63, 0.59], [0.29, 0.31, 0.61, 0.57], [0.30, 0.31, 0.62, 0.59],   # one object
    ], np.float32)
    rois = np.concatenate(parts + [fixed]).astype(np.float32)
    return rois[rng.permutation(len(rois))]


def main():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    reference = mg.load_reference()
    refc, rmodel = reference[0], reference[4]
    area = float(IMAGE_SHAPE[0] * IMAGE_SHAPE[1])
    rois = make_rois()
    k = rc.unrounded_level(rois, area)
    finite = np.isfinite(k)
    assert bool((np.abs(k[finite, None] - np.array([2.5, 3.5, 4.5])[None]).min(1) >= 1e-3).all()), "a box too near a level boundary"
    with mg.mute_stdout():
        levels = reference_levels(rmodel, rois)
    assert np.array_equal(levels[finite], rc.levels_of(rois[finite], area)), "the reference's levels differ from float64's"
    assert sorted(set(levels.tolist())) == [2, 3, 4, 5], levels.tolist()
    # the coverage the fixture promises
    assert bool(((rois < 0) | (rois > 1)).any(1).sum() >= 3)
    assert bool(((rois[:, 0] == rois[:, 2]) & (rois[:, 1] == rois[:, 3])).any())
    on_line = 0
    for box, lv in zip(rois, levels.tolist()):
        h, w = MAP_SIZES[lv - 2]
        for c1, c2, size in ((box[0], box[2], h), (box[1], box[3], w)):
            lo, hi, lerp, inside = rc.samples(c1, c2, size, 7)
            on_line += int((inside & (lerp == 0) & (lo == hi)).sum())
    assert on_line >= 8, on_line
    arrays = dict(image_shape=np.array(IMAGE_SHAPE), map_sizes=np.array(MAP_SIZES), rois=rois, levels=levels)
    rng = np.random.default_rng(7)
    for pool in POOLS:
        grad = ((rng.integers(-8, 8, (len(rois), pool, pool, CHANNELS[pool])) + 0.5) / 4.0).astype(np.float32)
        nchw = torch.from_numpy(grad).permute(0, 3, 1, 2).contiguous()
        with mg.mute_stdout():
            grads = reference_backward(refc, rois, levels, nchw)
        arrays[f"grad_out_p{pool}"] = grad
        for l, g in enumerate(grads):
            arrays[f"g{l}_p{pool}"] = g.permute(0, 2, 3, 1).contiguous().numpy()
            assert np.isfinite(arrays[f"g{l}_p{pool}"]).all() and np.count_nonzero(arrays[f"g{l}_p{pool}"]), (l, pool)
    arrays.update(numpy_version=np.array(np.__version__), torch_version=np.array(torch.__version__))
    mg.save("roi_align_backward", **arrays)

    # the tests' own reference (the committed C restatement) against what was just stored
    from oracle import oracle
    oracle.build()
    for pool in POOLS:
        want = rc.expected(oracle, arrays[f"grad_out_p{pool}"], rois, arrays["levels"], 1, MAP_SIZES, rois_per_image=len(rois))
        for l in range(4):
            assert np.array_equal(want[l].numpy().view(np.int32), arrays[f"g{l}_p{pool}"].view(np.int32)), (l, pool)
    print("tests/roi_align_backward_cases.expected reproduces the fixture bit for bit")


if __name__ == "__main__":
    main()
