// What csrc/losses.hip and csrc/mask_train.hip share, so that the mask loss on class planes is the dense mask loss bit for bit:
// binary cross entropy and its derivative in fp64, a slot's sum of terms, and the scale of a loss gradient. Function templates
// and inline functions only; the rule is stated at mrcnn_rpn_loss_forward in include/maskrcnn_hip.h.
#pragma once
#include <cmath>

#include "common.hpp"
#include "workgroup.hpp"

namespace mrcnn {

// log(1 - p) as torch takes it, log1p(-p): the same number wherever 1 - p is exact in fp64 (every fp32 p >= 2^-29, and 0)
__device__ __forceinline__ double bce(double p, double y) { return -(y * fmax(log(p), -100.0) + (1.0 - y) * fmax(log1p(-p), -100.0)); }

__device__ __forceinline__ double bce_grad(double p, double y) { return (p - y) / fmax((1.0 - p) * p, 1e-12); }

// The sum of a slot's hw mask terms, in every thread: thread t adds elements t, t + kThreads, ... from +0, then block_sum.
// Barriers: block_sum's two; every thread of the workgroup calls it.
template <int kThreads>
__device__ __forceinline__ double bce_slot_sum(const float* pm, const float* tm, int hw, double* red) {
    double acc = 0.0;
    for (int i = (int)threadIdx.x; i < hw; i += kThreads) acc += bce((double)pm[i], (double)tm[i]);
    return block_sum<kThreads>(acc, red);
}

// gradient scale of one loss: upstream gradient / count, 0 for a loss without a contributing element
__device__ __forceinline__ double grad_scale(float upstream, long long n) { return n > 0 ? (double)upstream / (double)n : 0.0; }

// the count a gradient is divided by: the image's own (per_image) or the batch's, summed here from counts[batch][kLosses]
template <int kLosses, int kThreads>
__device__ __forceinline__ void loss_scales(const int32_t* counts, const float* grad_out, int per_image, int batch, int b, long long* red,
                                            double* scale) {
#pragma unroll
    for (int k = 0; k < kLosses; ++k) {
        if (per_image) {
            scale[k] = grad_scale(grad_out[(int64_t)b * kLosses + k], counts[(int64_t)b * kLosses + k]);
        } else {
            long long n = 0;
            for (int i = (int)threadIdx.x; i < batch; i += kThreads) n += counts[(int64_t)i * kLosses + k];
            scale[k] = grad_scale(grad_out[k], block_sum<kThreads>(n, red));
        }
    }
}

}  // namespace mrcnn
