// The arithmetic of Pillow's 8-bit BILINEAR resample (Image.resize), shared by csrc/image.hip and csrc/gt_masks.hip:
// double-precision triangle-filter coefficients with the support stretched by the scale factor when shrinking, normalised,
// rounded to 22-bit fixed point; each pass is (2^21 + sum in*k) >> 22 clamped to [0,255]. Operation by operation in fp64:
// every translation unit that includes this is built with FP contraction off.
#pragma once
#include <hip/hip_runtime.h>

namespace mrcnn_resample {

constexpr int PRECISION_BITS = 32 - 8 - 2;

struct Axis {  // one resample direction
    int in_size, out_size, ksize;
    double scale, support, ss;  // ss = 1 / filterscale
};

__host__ __device__ inline Axis make_axis(int in_size, int out_size) {
    Axis a;
    a.in_size = in_size;
    a.out_size = out_size;
    double filterscale = a.scale = static_cast<double>(static_cast<float>(in_size)) / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    a.support = 1.0 * filterscale;  // BILINEAR support = 1.0
    a.ksize = static_cast<int>(ceil(a.support)) * 2 + 1;
    a.ss = 1.0 / filterscale;
    return a;
}

__device__ __forceinline__ double tri(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// Coefficients of output sample xx: first input tap, tap count, and k[0..ksize) (stride kstride ints).
__device__ __forceinline__ void axis_coeffs(const Axis& a, int xx, int& xmin, int& cnt, int* k, int kstride) {
    const double center = (xx + 0.5) * a.scale;
    xmin = static_cast<int>(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = static_cast<int>(center + a.support + 0.5);
    if (xmax > a.in_size) xmax = a.in_size;
    cnt = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < cnt; ++x) ww += tri((x + xmin - center + 0.5) * a.ss);
    for (int x = 0; x < cnt; ++x) {
        double w = tri((x + xmin - center + 0.5) * a.ss);
        if (ww != 0.0) w /= ww;
        k[x * kstride] = static_cast<int>(0.5 + w * static_cast<double>(1 << PRECISION_BITS));
    }
    for (int x = cnt; x < a.ksize; ++x) k[x * kstride] = 0;
}

__device__ __forceinline__ unsigned clip8(int v) {
    v >>= PRECISION_BITS;
    return static_cast<unsigned>(v < 0 ? 0 : v > 255 ? 255 : v);
}
// clip8 for values that are PACKED into a word (b0 | b1 << 8 | ...): the compiler fuses two shift + clamp + pack steps into
// gfx950's v_ashr_pk_u8_i32, whose result it then ORs the next bytes onto as if bits 16-31 were zero — on the MI355X they are
// not (they keep what the destination register held: measured, round 5: bytes 2 and 3 of every packed word came out OR-ed with
// stale bits). Making each clamped value opaque before it is shifted into place keeps the plain shift / clamp / or sequence.
__device__ __forceinline__ unsigned clip8_for_packing(int v) {
    unsigned c = clip8(v);
    asm volatile("" : "+v"(c));
    return c;
}

}  // namespace mrcnn_resample
