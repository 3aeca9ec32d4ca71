// Clipped SGD for a table of tensors: the global gradient norm, clip_grad_norm_'s coefficient and the momentum step (gfx950).
// The rule is stated at mrcnn_optim_clip_coef in include/maskrcnn_hip.h. Built with -ffp-contract=off: every product and sum
// below is its own fp64 rounding, as the rule states.
//
// A tile is kTile consecutive elements of ONE tensor; workgroup = tile. Thread t of a tile owns the kVecs groups of four elements
// at (i * kBlock + t) * 4, i = 0 .. kVecs - 1: a wave reads 1 KiB in a row with 16-byte loads where the tensor's base addresses
// allow them, and the same elements one by one where they do not, so both forms add and round the same values in the same order.
#include <cmath>

#include "common.hpp"
#include "workgroup.hpp"

namespace {

using mrcnn::kWave;

constexpr int kBlock = 256;
constexpr int kVecs = 4;
constexpr int kTile = kBlock * kVecs * 4;   // 4096 elements: 16 KiB of each of p, g and b
constexpr int kFinish = 256;
constexpr int kMaxTensors = 65535;
constexpr int64_t kMaxTiles = (int64_t)1 << 24;
constexpr int kModeClip = 0, kModeStepZero = 2;   // 1: step

// The table holds addresses as integers; a pointer made from one is a flat pointer to the compiler, which costs every access the
// LDS aperture check and a second wait counter. They are device memory: say so.
typedef __attribute__((address_space(1))) float gfloat;
typedef float vec4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) vec4f gvec4f;

struct Tile {
    gfloat* p;
    gfloat* g;
    gfloat* b;
    double wd;
    int count;   // elements of this tile, 0 for a tensor without a gradient (and for a tile the table does not cover)
    bool vec;    // p, g and b all on 16-byte boundaries; a tile starts a multiple of 16 KiB behind them
};

// The tensor of tile `tile`: the t with tile_off[t] <= tile < tile_off[t + 1], which skips the tensors without a tile. Uniform
// over the workgroup. tile_off[0] = 0 <= tile < tiles = tile_off[tensors].
__device__ __forceinline__ int find_tensor(const int64_t* __restrict__ tile_off, int tensors, int64_t tile) {
    int lo = 0, hi = tensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_off[mid] <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ Tile find_tile(const int64_t* __restrict__ table, const double* __restrict__ wd,
                                          const int64_t* __restrict__ tile_off, int tensors) {
    const int64_t tile = blockIdx.x;
    const int t = find_tensor(tile_off, tensors, tile);
    const int64_t* row = table + 4 * (int64_t)t;
    const int64_t pa = row[0], ga = row[1], ba = row[2], numel = row[3];
    const int64_t first = (tile - tile_off[t]) * kTile;   // 64-bit element offset
    const int64_t left = numel - first;
    Tile r;
    r.p = (gfloat*)pa + first;
    r.g = (gfloat*)ga + first;
    r.b = (gfloat*)ba + first;
    r.wd = wd ? wd[t] : 0.0;
    r.count = ga == 0 || left <= 0 ? 0 : (int)(left < kTile ? left : kTile);
    r.vec = ((pa | ga | ba) & 15) == 0;
    return r;
}

struct Quad {
    float v[4];
};

// Elements [at, at + 4) of a tile with `count` elements; the ones past the tile's end read as +0 and are not loaded.
__device__ __forceinline__ Quad load_quad(const gfloat* base, int at, int count, bool vec) {
    Quad q;
    if (vec && at + 4 <= count) {
        const vec4f x = *(const gvec4f*)(base + at);
        q.v[0] = x.x; q.v[1] = x.y; q.v[2] = x.z; q.v[3] = x.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) q.v[j] = at + j < count ? base[at + j] : 0.0f;
    }
    return q;
}

__device__ __forceinline__ void store_quad(gfloat* base, int at, int count, bool vec, const Quad& q) {
    if (vec && at + 4 <= count) {
        vec4f x;
        x.x = q.v[0]; x.y = q.v[1]; x.z = q.v[2]; x.w = q.v[3];
        *(gvec4f*)(base + at) = x;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (at + j < count) base[at + j] = q.v[j];
    }
}

// part[tile] = the tile's sum of double(g) * double(g): each thread its 16 elements in ascending order, then block_sum over the
// threads. A tile without a gradient stores +0, so the finishing sum needs no table.
__global__ __launch_bounds__(kBlock) void optim_sumsq_kernel(const int64_t* __restrict__ table, const int64_t* __restrict__ tile_off,
                                                             int tensors, double* __restrict__ part) {
    __shared__ double s_red[kBlock / kWave];
    const Tile t = find_tile(table, nullptr, tile_off, tensors);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < kVecs; ++i) {
        const int at = (i * kBlock + (int)threadIdx.x) * 4;
        if (at < t.count) {
            const Quad g = load_quad(t.g, at, t.count, t.vec);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += (double)g.v[j] * (double)g.v[j];
        }
    }
    const double total = mrcnn::block_sum<kBlock>(acc, s_red);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// S = the partials in index order: thread t adds the run [t * chunk, (t + 1) * chunk), block_sum adds the runs in thread order.
// info = (S, norm, c), status bit 0 = S is not finite.
__global__ __launch_bounds__(kFinish) void optim_finish_kernel(const double* __restrict__ part, int64_t tiles, double max_norm,
                                                               double* __restrict__ info, int32_t* __restrict__ status) {
    __shared__ double s_red[kFinish / kWave];
    const int64_t chunk = (tiles + kFinish - 1) / kFinish;
    const int64_t lo = min((int64_t)threadIdx.x * chunk, tiles), hi = min(lo + chunk, tiles);
    double acc = 0.0;
    for (int64_t i = lo; i < hi; ++i) acc += part[i];
    const double s = mrcnn::block_sum<kFinish>(acc, s_red);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s);
        const double q = max_norm / (norm + 1e-6);
        info[0] = s;
        info[1] = norm;
        info[2] = q < 1.0 ? q : 1.0;
        status[0] = isfinite(s) ? 0 : 1;
    }
}

struct ApplyParams {
    const int64_t* table;
    const double* wd;
    const int64_t* tile_off;
    const double* info;
    const int32_t* status;
    double lr, momentum;
    int tensors, mode;
};

__global__ __launch_bounds__(kBlock) void optim_apply_kernel(ApplyParams a) {
    const Tile t = find_tile(a.table, a.wd, a.tile_off, a.tensors);
    if (t.count == 0) return;
    const bool bad = a.status && (a.status[0] & 1);
    if (bad && a.mode != kModeStepZero) return;
    const double c = a.info ? a.info[2] : 1.0;
    const bool write_g = a.mode == kModeStepZero || c != 1.0;   // fp32(1 * g) is g: that store would not change a bit
#pragma unroll
    for (int i = 0; i < kVecs; ++i) {
        const int at = (i * kBlock + (int)threadIdx.x) * 4;
        if (at >= t.count) continue;
        Quad g;
        if (bad) {
            g.v[0] = g.v[1] = g.v[2] = g.v[3] = 0.0f;
        } else {
            g = load_quad(t.g, at, t.count, t.vec);
            if (a.mode != kModeClip) {
                Quad p = load_quad(t.p, at, t.count, t.vec), b = load_quad(t.b, at, t.count, t.vec);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = c * (double)g.v[j] + t.wd * (double)p.v[j];
                    const double nb = a.momentum * (double)b.v[j] + d;
                    b.v[j] = (float)nb;
                    p.v[j] = (float)((double)p.v[j] - a.lr * nb);
                }
                store_quad(t.p, at, t.count, t.vec, p);
                store_quad(t.b, at, t.count, t.vec, b);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) g.v[j] = a.mode == kModeStepZero ? 0.0f : (float)(c * (double)g.v[j]);
        }
        if (write_g) store_quad(t.g, at, t.count, t.vec, g);
    }
}

int check_table(const char* who, const void* table, const void* tile_off, int32_t tensors, int64_t tiles) {
    MRCNN_REQUIRE(table && tile_off, "%s: null pointer", who);
    MRCNN_REQUIRE(tensors >= 1 && tensors <= kMaxTensors, "%s: num_tensors=%d must be in [1, %d]", who, tensors, kMaxTensors);
    MRCNN_REQUIRE(tiles >= 0 && tiles <= kMaxTiles, "%s: tiles=%lld must be in [0, %lld]", who, (long long)tiles, (long long)kMaxTiles);
    return MRCNN_OK;
}

}  // namespace

extern "C" int32_t mrcnn_optim_tile(void) { return kTile; }

extern "C" int mrcnn_optim_clip_coef(const int64_t* table, const int64_t* tile_off, int32_t num_tensors, int64_t tiles, double max_norm,
                                     double* workspace, double* info, int32_t* status, mrcnn_stream_t stream) {
    const char* who = "optim_clip_coef";
    if (int rc = check_table(who, table, tile_off, num_tensors, tiles)) return rc;
    MRCNN_REQUIRE(workspace && info && status, "%s: null pointer", who);
    MRCNN_REQUIRE(max_norm > 0.0, "%s: max_norm=%g must be above 0", who, max_norm);
    MRCNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(info) & 7) == 0,
                  "%s: the workspace and info must be 8-byte aligned", who);
    hipStream_t s = mrcnn::as_stream(stream);
    if (tiles > 0)
        hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, s, table, tile_off, num_tensors, workspace);
    hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(kFinish), 0, s, workspace, tiles, max_norm, info, status);
    return mrcnn::check_launch(who);
}

extern "C" int mrcnn_optim_sgd_apply(const int64_t* table, const double* wd, const int64_t* tile_off, int32_t num_tensors, int64_t tiles,
                                     const double* info, const int32_t* status, double lr, double momentum, int32_t mode,
                                     mrcnn_stream_t stream) {
    const char* who = "optim_sgd_apply";
    if (int rc = check_table(who, table, tile_off, num_tensors, tiles)) return rc;
    MRCNN_REQUIRE(wd, "%s: null pointer", who);
    MRCNN_REQUIRE(std::isfinite(lr), "%s: lr=%g must be finite", who, lr);
    MRCNN_REQUIRE(momentum >= 0.0 && momentum < 1.0, "%s: momentum=%g must be in [0, 1)", who, momentum);
    MRCNN_REQUIRE(mode >= kModeClip && mode <= kModeStepZero, "%s: mode=%d must be 0 (clip), 1 (step) or 2 (step_zero)", who, mode);
    if (tiles == 0) return MRCNN_OK;
    ApplyParams a;
    a.table = table; a.wd = wd; a.tile_off = tile_off; a.info = info; a.status = status;
    a.lr = lr; a.momentum = momentum; a.tensors = num_tensors; a.mode = mode;
    hipLaunchKernelGGL(optim_apply_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, mrcnn::as_stream(stream), a);
    return mrcnn::check_launch(who);
}
