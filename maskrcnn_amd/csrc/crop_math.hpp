// The arithmetic of crop_and_resize (crop_cpu.cpp:13-116 of the reference), shared by csrc/crop.hip and
// csrc/detection_targets.hip: one sample coordinate per crop row / column and the a+(b-a)*t lerps, operation by operation.
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

}  // namespace mrcnn_crop
