// The matching rule of the two training-target steps (data.rpn_samples, data.py:485-540, and model.mrn_samples, model.py:396-576),
// shared by csrc/targets.hip and csrc/detection_targets.hip: which rows of an image are its own, which of them are kept, the fp32
// IoU of boxes_overlaps (data.py:151-189) operation by operation, and the walk that keeps max / first argmax / crowd max.
// Every translation unit that includes this is built with FP contraction off.
#pragma once
#include "common.hpp"

namespace mrcnn_match {

constexpr int kMaxRows = 1024;             // rows of one image (LDS; 10 bits of detection_targets' sort key)
constexpr int kMaxBatch = 65535;           // an image is a grid row

// Host side, first in every entry point that takes packed rows: the batch and row limits, in one wording.
inline int check_rows(const char* who, int32_t num_rows, int32_t batch) {
    MRCNN_REQUIRE(batch >= 1 && batch <= kMaxBatch, "%s: batch=%d must be in [1, %d]", who, batch, kMaxBatch);
    MRCNN_REQUIRE(num_rows >= 0 && (int64_t)num_rows <= (int64_t)kMaxRows * batch,
                  "%s: num_rows=%d must be in [0, %d * batch]: at most %d rows per image", who, num_rows, kMaxRows, kMaxRows);
    return MRCNN_OK;
}

struct Rows {
    int start, n;
};

// rows of image b, whatever gt_off holds: inside [0, m] and at most kMaxRows of them
__device__ __forceinline__ Rows image_rows(const int32_t* gt_off, int b, int m) {
    const int s = min(max(gt_off[b], 0), m);
    const int e = min(max(gt_off[b + 1], s), m);
    return Rows{s, min(e - s, kMaxRows)};
}

// crowd rule, quirk included (data.py:496-502, model.py:435-442): with a crowd row (id < 0) in the image, rows with id > 0 are
// kept and id 0 is dropped; without one every row is kept
__device__ __forceinline__ bool row_kept(int id, bool image_has_crowd) { return image_has_crowd ? id > 0 : true; }

__device__ __forceinline__ float box_area(float4 b) { return (b.z - b.x) * (b.w - b.y); }   // (y1, x1, y2, x2)

// IoU of box a with row g, the areas as box_area gives them: each operation separately rounded, (a_area + g_area) - inter in
// that order, correctly rounded division. 0 / 0 (two empty boxes) is NaN, as in the reference.
__device__ __forceinline__ float box_iou(float4 a, float a_area, float4 g, float g_area) {
    const float y1 = fmaxf(a.x, g.x), x1 = fmaxf(a.y, g.y), y2 = fminf(a.z, g.z), x2 = fminf(a.w, g.w);
    const float inter = fmaxf(x2 - x1, 0.f) * fmaxf(y2 - y1, 0.f);
    const float uni = (a_area + g_area) - inter;
    return inter / uni;
}

// One box's walk over the rows of its image, in row order:
//     if (row_kept(id, crowd)) walk.kept_row(g, iou); else if (id < 0) walk.crowd_row(iou);      (a dropped id-0 row counts nowhere)
// The two row loops spell that line themselves: anchor_match's wave reduction belongs inside its kept branch, and a combined
// function that hands the flag back made the compiler branch on it twice — 4 % on anchor_match, measured.
struct Match {
    float best = -1.f, crowd_max = 0.f;   // the largest IoU with a kept row, with a crowd row
    int arg = -1;                         // the kept row of `best`; -1: no kept row yet

    // the FIRST largest wins, as np.argmax and torch.max(dim=1); a NaN never wins (no comparison with it holds)
    __device__ __forceinline__ void kept_row(int g, float iou) {
        if (iou > best) {
            best = iou;
            arg = g;
        }
    }
    __device__ __forceinline__ void crowd_row(float iou) { crowd_max = fmaxf(crowd_max, iou); }
};

}  // namespace mrcnn_match
