// The arithmetic of crop_and_resize (crop_cpu.cpp:13-116 of the reference), shared by csrc/crop.hip, csrc/roi_align_backward.hip
// and csrc/detection_targets.hip: one sample coordinate per crop row / column and the a+(b-a)*t lerps, operation by operation;
// and the pyramid level of a RoI (model.py:324-338).
// Every translation unit that includes this is built with FP contraction off.
#pragma once
#include <hip/hip_runtime.h>

namespace mrcnn_crop {

struct Sample {   // one crop row or column
    int lo, hi;   // tap indices (floorf / ceilf)
    float lerp;   // in - lo
    int inside;   // 0 → extrapolation_value
};

// crop_cpu.cpp:52-61 (y) and :82-84 (x): identical formulas with (c1,c2,size,crop) swapped in.
__device__ __forceinline__ Sample make_sample(float c1, float c2, int size, int crop, int t) {
    float in;
    if (crop > 1) {
        float s = c2 - c1;
        s = s * static_cast<float>(size - 1);
        const float scale = s / static_cast<float>(crop - 1);
        const float a = c1 * static_cast<float>(size - 1);
        const float b = static_cast<float>(t) * scale;
        in = a + b;
    } else {  // 0.5 * (c1 + c2) * (size - 1): the literal is double in the reference
        const float sum = c1 + c2;
        in = static_cast<float>(0.5 * static_cast<double>(sum) * static_cast<double>(size - 1));
    }
    Sample r;
    r.inside = !(in < 0.0f || in > static_cast<float>(size - 1));
    r.lo = r.inside ? static_cast<int>(floorf(in)) : 0;
    r.hi = r.inside ? static_cast<int>(ceilf(in)) : 0;
    r.lerp = in - static_cast<float>(r.lo);
    return r;
}

__device__ __forceinline__ float bilerp(float tl, float tr, float bl, float br, float xl, float yl) {
    float t = tr - tl;
    t = t * xl;
    const float top = tl + t;
    float u = br - bl;
    u = u * xl;
    const float bot = bl + u;
    float v = bot - top;
    v = v * yl;
    return top + v;
}

// The pyramid's maps and the level of a RoI (csrc/crop.hip's forward and csrc/roi_align_backward.hip: one definition, so that the two
// cannot disagree about a box).
struct PyramidArgs {
    const float* fm[4];
    int h[4], w[4];
};

__device__ __forceinline__ int roi_level(float y1, float x1, float y2, float x2, float image_area) {
    // model.py:324-338 in fp32: 4 + log2(sqrt(h*w) / (224 / sqrt(area))), round half to even, clamp.
    // Every fp32 operation of that formula is evaluated CORRECTLY ROUNDED: sqrt, the two divisions and log2 go through
    // double and are rounded to float once (exact for sqrt and division, 53 >= 2*24 + 2; for log2 up to double's own
    // error, ~1e-8 of the inputs). torch-CPU's log2 (MKL VML, high-accuracy mode) is correctly rounded on all but
    // ~1e-4 of its inputs, the device's log2f on far fewer: with log2f 7-11 % of the boxes within a few ulp of a level
    // boundary k = 2.5 / 3.5 / 4.5 landed one level off (tests/test_gpu_fullsize.py::test_level_boundaries_ulp_sweep).
    const float h = y2 - y1, w = x2 - x1;
    const float hw = h * w;
    const float denom = static_cast<float>(224.0 / static_cast<double>(static_cast<float>(sqrt(static_cast<double>(image_area)))));
    const float ratio = static_cast<float>(static_cast<double>(static_cast<float>(sqrt(static_cast<double>(hw)))) /
                                           static_cast<double>(denom));
    const float k = 4.0f + static_cast<float>(log2(static_cast<double>(ratio)));
    // NaN (negative area) / -inf (zero area) → the reference's int cast is UB; it lands on level 2
    if (!(k >= 2.0f)) return 2;
    if (k >= 5.0f) return 5;
    return static_cast<int>(rintf(k));
}

}  // namespace mrcnn_crop
