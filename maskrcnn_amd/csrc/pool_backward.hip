// The two gradient kernels of the backbone that are not convolutions; the rules are stated at mrcnn_dilate2_sum_f32 and
// mrcnn_maxpool_backward_f32 in include/maskrcnn_hip.h. Built with -ffp-contract=off: every add here is its own fp32 operation.
//   dilate2_sum        compact [B][OH][OW][C] (one tensor, or the fp32 sum of two) -> dx [B][H][W][C], OH = ceil(H / 2): the values
//                      at the even positions, +0 everywhere else. The data gradient of a 1 x 1 stride-2 conv from its compact form
//                      (two of them where conv1 and the downsample conv of a block read the same x), and the backward of P6's
//                      MaxPool2d(1, 2). A thread owns one 16-byte quad of dx and stores it once.
//   maxpool_backward   the gather form of the zero-padded max-pool's backward: a thread owns one channel quad of one input pixel,
//                      recomputes the argmax of the at most ceil(k/s)^2 windows that cover it from the saved input and adds the
//                      gradients of those that take it, in ascending (oy, ox) order from +0.
// No atomic, no memset, no LDS, no barrier; nothing here synchronises with the host.
#include "common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr long long kMaxBytes = 0xFFFFFFF0LL;   // every tensor: element offsets stay far inside 32 bits

struct DilateParams {
    const float* a;
    const float* b2;   // or null
    float* dx;
    int H, W, OH, OW, Q;   // Q: channel quads
    long long quads;       // B * H * W * Q
};

__global__ __launch_bounds__(kThreads) void dilate2_sum(const DilateParams p) {
    const long long e = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x;
    if (e >= p.quads) return;
    const int q = static_cast<int>(e % p.Q);
    long long r = e / p.Q;
    const int ix = static_cast<int>(r % p.W);
    r /= p.W;
    const int iy = static_cast<int>(r % p.H), b = static_cast<int>(r / p.H);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!((iy | ix) & 1)) {   // (iy / 2, ix / 2) is inside the compact map: OH = ceil(H / 2), OW = ceil(W / 2)
        const size_t src = ((static_cast<size_t>(b) * p.OH + (iy >> 1)) * p.OW + (ix >> 1)) * p.Q + q;
        v = reinterpret_cast<const float4*>(p.a)[src];
        if (p.b2) {
            const float4 t = reinterpret_cast<const float4*>(p.b2)[src];
            v.x = v.x + t.x; v.y = v.y + t.y; v.z = v.z + t.z; v.w = v.w + t.w;
        }
    }
    reinterpret_cast<float4*>(p.dx)[e] = v;
}

struct PoolBackwardParams {
    const float* dy;   // [B][OH][OW][C]
    const float* x;    // [B][H][W][C]
    float* dx;
    int H, W, OH, OW, Q, k, s, pt, pl;
    long long quads;
};

__device__ __forceinline__ bool takes(float v, float best) { return v > best || v != v; }

__global__ __launch_bounds__(kThreads) void maxpool_backward(const PoolBackwardParams p) {
    const long long e = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x;
    if (e >= p.quads) return;
    const int q = static_cast<int>(e % p.Q);
    long long r = e / p.Q;
    const int ix = static_cast<int>(r % p.W);
    r /= p.W;
    const int iy = static_cast<int>(r % p.H), b = static_cast<int>(r / p.H);
    const float4* x4 = reinterpret_cast<const float4*>(p.x) + static_cast<size_t>(b) * p.H * p.W * p.Q + q;
    const float4* g4 = reinterpret_cast<const float4*>(p.dy) + static_cast<size_t>(b) * p.OH * p.OW * p.Q + q;
    // the windows that cover (iy, ix): oy * s - pt <= iy <= oy * s - pt + k - 1
    const int ty = iy + p.pt, tx = ix + p.pl;
    const int oy0 = ty < p.k ? 0 : (ty - p.k + p.s) / p.s, oy1 = min(ty / p.s, p.OH - 1);
    const int ox0 = tx < p.k ? 0 : (tx - p.k + p.s) / p.s, ox1 = min(tx / p.s, p.OW - 1);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int oy = oy0; oy <= oy1; ++oy)
        for (int ox = ox0; ox <= ox1; ++ox) {
            const int y0 = oy * p.s - p.pt, x0 = ox * p.s - p.pl;
            const int mine = (iy - y0) * p.k + (ix - x0);   // this thread's tap of the window
            // torch's walk: max = -inf at the window's first tap, then `val > max || isnan(val)` in (ky, kx) order
            float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            int arg[4] = {0, 0, 0, 0};
            for (int ky = 0; ky < p.k; ++ky)
                for (int kx = 0; kx < p.k; ++kx) {
                    const int yy = y0 + ky, xx = x0 + kx;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);   // a padding tap reads 0
                    if (static_cast<unsigned>(yy) < static_cast<unsigned>(p.H) && static_cast<unsigned>(xx) < static_cast<unsigned>(p.W))
                        v = x4[(static_cast<size_t>(yy) * p.W + xx) * p.Q];
                    const float vv[4] = {v.x, v.y, v.z, v.w};
                    const int tap = ky * p.k + kx;
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (takes(vv[c], best[c])) {
                            best[c] = vv[c];
                            arg[c] = tap;
                        }
                }
            const float4 g = g4[(static_cast<size_t>(oy) * p.OW + ox) * p.Q];
            const float gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (arg[c] == mine) acc[c] = acc[c] + gg[c];
        }
    reinterpret_cast<float4*>(p.dx)[e] = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int mrcnn_dilate2_sum_f32(const float* a, const float* b2, int32_t batch, int32_t height, int32_t width, int32_t channels,
                                     float* dx, mrcnn_stream_t stream) {
    const char* who = "dilate2_sum";
    MRCNN_REQUIRE(batch >= 1 && height >= 1 && width >= 1 && channels >= 4 && channels % 4 == 0,
                  "%s: bad shape B=%d H=%d W=%d C=%d (C %% 4 == 0 required)", who, batch, height, width, channels);
    const long long elems = 1LL * batch * height * width * channels;
    MRCNN_REQUIRE(4 * elems <= kMaxBytes, "%s: tensor too large (dx <= 0xFFFFFFF0 bytes)", who);
    MRCNN_REQUIRE(a && dx, "%s: null pointer", who);
    MRCNN_REQUIRE(aligned16(a) && aligned16(b2) && aligned16(dx), "%s: the tensors must lie on 16-byte boundaries", who);
    DilateParams p;
    p.a = a; p.b2 = b2; p.dx = dx; p.H = height; p.W = width; p.OH = (height + 1) / 2; p.OW = (width + 1) / 2; p.Q = channels / 4;
    p.quads = elems / 4;
    hipLaunchKernelGGL(dilate2_sum, dim3(static_cast<unsigned>((p.quads + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       mrcnn::as_stream(stream), p);
    return mrcnn::check_launch("dilate2_sum");
}

extern "C" int mrcnn_maxpool_backward_f32(const float* dy, const float* x, int32_t batch, int32_t height, int32_t width,
                                          int32_t channels, int32_t kernel, int32_t stride, int32_t pad_top, int32_t pad_left,
                                          int32_t pad_bottom, int32_t pad_right, float* dx, mrcnn_stream_t stream) {
    const char* who = "maxpool_backward";
    MRCNN_REQUIRE(batch >= 1 && height >= 1 && width >= 1 && channels >= 4 && channels % 4 == 0,
                  "%s: bad shape B=%d H=%d W=%d C=%d (C %% 4 == 0 required)", who, batch, height, width, channels);
    MRCNN_REQUIRE(kernel >= 1 && kernel <= 3 && stride >= 1 && stride <= 2, "%s: kernel must be in 1 .. 3 and stride in 1 .. 2, got %d and %d",
                  who, kernel, stride);
    MRCNN_REQUIRE(pad_top >= 0 && pad_left >= 0 && pad_bottom >= 0 && pad_right >= 0 && pad_top < kernel && pad_left < kernel &&
                      pad_bottom < kernel && pad_right < kernel,
                  "%s: every pad must be in 0 .. kernel - 1", who);
    MRCNN_REQUIRE(height + pad_top + pad_bottom >= kernel && width + pad_left + pad_right >= kernel, "%s: empty output", who);
    const long long elems = 1LL * batch * height * width * channels;
    MRCNN_REQUIRE(4 * elems <= kMaxBytes, "%s: tensor too large (x <= 0xFFFFFFF0 bytes)", who);
    MRCNN_REQUIRE(dy && x && dx, "%s: null pointer", who);
    MRCNN_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(dx), "%s: the tensors must lie on 16-byte boundaries", who);
    PoolBackwardParams p;
    p.dy = dy; p.x = x; p.dx = dx; p.H = height; p.W = width; p.Q = channels / 4; p.k = kernel; p.s = stride; p.pt = pad_top; p.pl = pad_left;
    p.OH = (height + pad_top + pad_bottom - kernel) / stride + 1;
    p.OW = (width + pad_left + pad_right - kernel) / stride + 1;
    p.quads = elems / 4;
    hipLaunchKernelGGL(maxpool_backward, dim3(static_cast<unsigned>((p.quads + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       mrcnn::as_stream(stream), p);
    return mrcnn::check_launch("maxpool_backward");
}
