// The RPN's training branch on the sampled anchors alone (gfx950): the compaction of rpn_match, the gather of the 3x3xC patches under
// the sampled anchors' pixels out of the pyramid, and its backward, the scatter of the patch gradients into the pyramid. The rules are
// stated at mrcnn_anchor_compact, mrcnn_pyramid_patch_gather_f32 and mrcnn_pyramid_patch_scatter_f32 in include/maskrcnn_hip.h.
//
// Anchor order is rpn_scores_deltas' (csrc/misc.hip): anchor a = first[l] + (y * W_l + x) * apl + r, so an image's index row, which
// is ascending in a, is sorted by level, then map row, then pixel.
//   compact  one workgroup per image walks the image's match row 16 384 anchors at a time; the non-zero flags are scanned in thread
//            order (workgroup.hpp), so slot k is the k-th such anchor. It stops as soon as the row is known to overflow.
//   gather   one workgroup per patch row (b, k): 9 * C / 4 float4 copies, +0 for the padding taps and for an empty slot.
//   scatter  MAP-stationary, as the RoIAlign backward: one workgroup per (level, image, map row, 16 pixels). The entries that can
//            reach the strip lie in three contiguous ranges of the sorted index row, one per map row y-1, y, y+1, whose ends every
//            wave finds by counting the entries below six workgroup-uniform keys (ballots over the row). A thread owns 4 channels of one pixel and adds
//            the terms of the entries within one pixel of its own in ascending slot, from +0, and stores once. Nearly every strip
//            has three empty ranges and stores zeros: the floor is the plain fill of the maps.
#pragma clang fp contract(off)

#include "common.hpp"
#include "workgroup.hpp"

namespace {

constexpr int MAX_LEVELS = 8;
constexpr int MAX_SIDE = 16384;
constexpr int MAX_APL = 16;
constexpr int MAX_CAPACITY = 1024;
constexpr int MAX_BATCH = 65535;
constexpr long long MAX_ELEMENTS = 1LL << 30;   // a map or the patch matrix: the 4 GiB range the conv forward accepts

constexpr int COMPACT_THREADS = 1024;
constexpr int COMPACT_RUN = 16;      // consecutive anchors per thread and walk: 16 384 anchors a walk (4 per thread: 0.090 ms for
                                     // 2 x 261 888 anchors, a barrier pair every 4096; 16: see profiles/rpn_train_microbench.jsonl)
static_assert(COMPACT_RUN % 4 == 0, "whole int4 loads");
constexpr int THREADS = 256;
constexpr int STRIP = 16;            // pixels of a map row per scatter workgroup

struct Pyramid {
    float* map[MAX_LEVELS];          // gather: read only. scatter: the gradient maps, null = not asked for
    int h[MAX_LEVELS], w[MAX_LEVELS];
    int first[MAX_LEVELS + 1];       // the first anchor of level l; first[levels] = A
    int tile_first[MAX_LEVELS + 1];  // scatter: the first workgroup of level l
    int levels, apl;
};

struct Level {
    float* map;
    int h, w, first, tile_first, index;
};

// The last level l < levels with key >= at(l) (at is ascending): constant indices into the kernel argument only, no scratch.
template <bool kByTile>
__device__ __forceinline__ Level find_level(const Pyramid& p, int key) {
    Level r;
    r.map = p.map[0]; r.h = p.h[0]; r.w = p.w[0]; r.first = p.first[0]; r.tile_first = p.tile_first[0]; r.index = 0;
#pragma unroll
    for (int l = 1; l < MAX_LEVELS; ++l) {
        if (l < p.levels && key >= (kByTile ? p.tile_first[l] : p.first[l])) {
            r.map = p.map[l]; r.h = p.h[l]; r.w = p.w[l]; r.first = p.first[l]; r.tile_first = p.tile_first[l]; r.index = l;
        }
    }
    return r;
}

// grid = batch, block = 1024
__global__ __launch_bounds__(COMPACT_THREADS) void anchor_compact_kernel(
    const int* __restrict__ match, int num_anchors, int capacity, int* __restrict__ index, int* __restrict__ num,
    int* __restrict__ status) {
    __shared__ int red[COMPACT_THREADS / mrcnn::kWave];
    const int b = blockIdx.x;
    const int* m = match + static_cast<int64_t>(b) * num_anchors;
    int* out = index + static_cast<int64_t>(b) * capacity;
    const bool aligned = (reinterpret_cast<uintptr_t>(m) & 15) == 0;
    int seen = 0;   // anchors with match != 0 before `base`: the same in every thread
    for (int64_t base = 0; base < num_anchors && seen <= capacity; base += COMPACT_THREADS * COMPACT_RUN) {
        const int64_t a0 = base + threadIdx.x * COMPACT_RUN;   // a thread owns COMPACT_RUN consecutive anchors: thread order is anchor order
        int v[COMPACT_RUN];
        if (aligned && a0 + COMPACT_RUN <= num_anchors) {
#pragma unroll
            for (int q = 0; q < COMPACT_RUN / 4; ++q) {        // independent 16-byte loads: one memory latency per walk
                const int4 w = *reinterpret_cast<const int4*>(m + a0 + 4 * q);
                v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < COMPACT_RUN; ++j) v[j] = a0 + j < num_anchors ? m[a0 + j] : 0;
        }
        int mine = 0;
#pragma unroll
        for (int j = 0; j < COMPACT_RUN; ++j) mine += v[j] != 0;
        int total;
        int pos = seen + mrcnn::block_inclusive_scan<COMPACT_THREADS>(mine, red, total) - mine;
        if (mine) {
#pragma unroll
            for (int j = 0; j < COMPACT_RUN; ++j) {
                if (v[j] != 0) {
                    if (pos < capacity) out[pos] = static_cast<int>(a0 + j);
                    ++pos;
                }
            }
        }
        seen += total;
    }
    const int n = min(seen, capacity);
    for (int k = n + threadIdx.x; k < capacity; k += COMPACT_THREADS) out[k] = -1;
    if (threadIdx.x == 0) {
        num[b] = n;
        status[b] = seen > capacity ? 1 : 0;
    }
}

// grid = batch * capacity, block = 256
__global__ __launch_bounds__(THREADS) void patch_gather_kernel(Pyramid p, int c4, int capacity, const int* __restrict__ index,
                                                               const int* __restrict__ num, float4* __restrict__ patches) {
    const int row = blockIdx.x;
    const int b = row / capacity, k = row - b * capacity;
    int anchor = -1;
    if (k < num[b]) anchor = index[row];
    const bool live = anchor >= 0 && anchor < p.first[p.levels];
    const Level lv = find_level<false>(p, live ? anchor : 0);
    const int pix = (live ? anchor - lv.first : 0) / p.apl;
    const int py = pix / lv.w, px = pix - py * lv.w;
    const float4* src = reinterpret_cast<const float4*>(lv.map) + static_cast<int64_t>(b) * lv.h * lv.w * c4;
    float4* dst = patches + static_cast<int64_t>(row) * 9 * c4;
    for (int e = threadIdx.x; e < 9 * c4; e += THREADS) {
        const int tap = e / c4, c = e - tap * c4;
        const int ky = tap / 3, kx = tap - ky * 3;
        const int y = py + ky - 1, x = px + kx - 1;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live && y >= 0 && y < lv.h && x >= 0 && x < lv.w) v = src[(static_cast<int64_t>(y) * lv.w + x) * c4 + c];
        dst[e] = v;
    }
}

// grid = the strips of the requested levels, block = 256
__global__ __launch_bounds__(THREADS) void patch_scatter_kernel(Pyramid p, int c4, int capacity, const int* __restrict__ index,
                                                                const int* __restrict__ num, const float4* __restrict__ dpatch) {
    const Level lv = find_level<true>(p, static_cast<int>(blockIdx.x));
    const int H = lv.h, W = lv.w, strips = (W + STRIP - 1) / STRIP;
    int rem = static_cast<int>(blockIdx.x) - lv.tile_first;
    const int b = rem / (H * strips);
    rem -= b * (H * strips);
    const int y = rem / strips, x0 = (rem - y * strips) * STRIP;
    const int* idx = index + static_cast<int64_t>(b) * capacity;
    const int n = min(max(num[b], 0), capacity);

    // per map row y-1, y, y+1: the anchors of the pixels x0-1 .. x0+STRIP of that row are [key_lo, key_hi), the slots [s, e)
    int key_lo[3], key_hi[3], s[3], e[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int yy = y - 1 + r;
        key_lo[r] = key_hi[r] = s[r] = e[r] = 0;
        if (yy >= 0 && yy < H) {
            const int xlo = max(x0 - 1, 0), xhi = min(x0 + STRIP, W - 1);
            key_lo[r] = lv.first + (yy * W + xlo) * p.apl;
            key_hi[r] = lv.first + (yy * W + xhi + 1) * p.apl;
        }
    }
    // The first slot that holds `key` or more is the number of entries below it, the row being ascending. Every wave counts for
    // itself, 64 entries per load and a ballot per key: the loads are independent, so the six searches cost one memory latency where
    // six binary searches were 6 log2(n) dependent loads (0.077 ms against 0.036 for the plain fill of 179 MB of maps). The
    // counts are the same in every wave, and s <= e whatever the row holds.
    const int lane = threadIdx.x & (mrcnn::kWave - 1);
    for (int base = 0; base < n; base += mrcnn::kWave) {
        const int v = base + lane < n ? idx[base + lane] : 0x7FFFFFFF;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            s[r] += __popcll(__ballot(v < key_lo[r]));
            e[r] += __popcll(__ballot(v < key_hi[r]));
        }
    }
    float4* out = reinterpret_cast<float4*>(lv.map) + (static_cast<int64_t>(b) * H + y) * W * c4;
    const float4* g = dpatch + static_cast<int64_t>(b) * capacity * 9 * c4;
    const int width = min(STRIP, W - x0);
    for (int el = threadIdx.x; el < width * c4; el += THREADS) {
        const int dx = el / c4, c = el - dx * c4;
        const int x = x0 + dx;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            for (int k = s[r]; k < e[r]; ++k) {
                const int a = idx[k];
                if (a < key_lo[r] || a >= key_hi[r]) continue;     // a row that is not sorted: nothing is read through it
                const int pix = (a - lv.first) / p.apl;
                const int px = pix - (pix / W) * W;
                if (px < x - 1 || px > x + 1) continue;
                // the entry's pixel is (y - 1 + r, px): its tap on (y, x) is (ky, kx) = (2 - r, x - px + 1)
                const float4 t = g[(static_cast<int64_t>(k) * 9 + (2 - r) * 3 + (x - px + 1)) * c4 + c];
                acc.x = acc.x + t.x;
                acc.y = acc.y + t.y;
                acc.z = acc.z + t.z;
                acc.w = acc.w + t.w;
            }
        }
        out[static_cast<int64_t>(x) * c4 + c] = acc;
    }
}

// The checks and the anchor table the gather and the scatter share. maps: null entries are legal when `optional`.
int fill_pyramid(const char* who, Pyramid& p, float* const* maps, bool optional, const int32_t* map_h, const int32_t* map_w,
                 int32_t levels, int32_t batch, int32_t channels, int32_t apl, int32_t capacity, const void* index,
                 const void* num, const void* patches) {
    MRCNN_REQUIRE(levels >= 1 && levels <= MAX_LEVELS, "%s: levels=%d must be in 1 .. %d", who, levels, MAX_LEVELS);
    MRCNN_REQUIRE(maps && map_h && map_w && index && num && patches, "%s: null pointer", who);
    MRCNN_REQUIRE(batch >= 1 && batch <= MAX_BATCH, "%s: batch=%d must be in 1 .. %d", who, batch, MAX_BATCH);
    MRCNN_REQUIRE(channels >= 4 && channels % 4 == 0, "%s: channels=%d must be a multiple of 4", who, channels);
    MRCNN_REQUIRE(apl >= 1 && apl <= MAX_APL, "%s: anchors_per_location=%d must be in 1 .. %d", who, apl, MAX_APL);
    MRCNN_REQUIRE(capacity >= 1 && capacity <= MAX_CAPACITY, "%s: capacity=%d must be in 1 .. %d", who, capacity, MAX_CAPACITY);
    MRCNN_REQUIRE((reinterpret_cast<uintptr_t>(patches) & 15) == 0, "%s: the patch matrix must be 16-byte aligned", who);
    MRCNN_REQUIRE(9LL * channels * capacity * batch <= MAX_ELEMENTS, "%s: the patch matrix must hold at most 2^30 elements", who);
    long long anchors = 0;
    for (int l = 0; l < MAX_LEVELS; ++l) {
        p.map[l] = nullptr;
        p.h[l] = p.w[l] = 1;
        p.first[l] = p.tile_first[l] = 0x7FFFFFFF;
    }
    for (int l = 0; l < levels; ++l) {
        MRCNN_REQUIRE(map_h[l] >= 1 && map_h[l] <= MAX_SIDE && map_w[l] >= 1 && map_w[l] <= MAX_SIDE,
                      "%s: level %d: %d x %d must be in 1 .. %d a side", who, l, map_h[l], map_w[l], MAX_SIDE);
        MRCNN_REQUIRE(optional || maps[l], "%s: level %d: null pointer", who, l);
        MRCNN_REQUIRE((reinterpret_cast<uintptr_t>(maps[l]) & 15) == 0, "%s: level %d must be 16-byte aligned", who, l);
        MRCNN_REQUIRE(1LL * batch * map_h[l] * map_w[l] * channels <= MAX_ELEMENTS, "%s: level %d must hold at most 2^30 elements", who, l);
        p.map[l] = maps[l];
        p.h[l] = map_h[l];
        p.w[l] = map_w[l];
        p.first[l] = static_cast<int>(anchors);
        anchors += 1LL * map_h[l] * map_w[l] * apl;
        MRCNN_REQUIRE(anchors < (1LL << 31), "%s: the pyramid must hold fewer than 2^31 anchors", who);
    }
    p.first[levels] = static_cast<int>(anchors);
    p.levels = levels;
    p.apl = apl;
    return MRCNN_OK;
}

}  // namespace

extern "C" int mrcnn_anchor_compact(const int32_t* match, int32_t batch, int32_t num_anchors, int32_t capacity, int32_t* index,
                                    int32_t* num, int32_t* status, mrcnn_stream_t stream) {
    const char* who = "anchor_compact";
    MRCNN_REQUIRE(match && index && num && status, "%s: null pointer", who);
    MRCNN_REQUIRE(batch >= 1 && batch <= MAX_BATCH, "%s: batch=%d must be in 1 .. %d", who, batch, MAX_BATCH);
    MRCNN_REQUIRE(num_anchors >= 1 && 1LL * batch * num_anchors < (1LL << 31), "%s: batch * num_anchors must be below 2^31", who);
    MRCNN_REQUIRE(capacity >= 1 && capacity <= MAX_CAPACITY, "%s: capacity=%d must be in 1 .. %d", who, capacity, MAX_CAPACITY);
    hipLaunchKernelGGL(anchor_compact_kernel, dim3(batch), dim3(COMPACT_THREADS), 0, mrcnn::as_stream(stream), match, num_anchors,
                       capacity, index, num, status);
    return mrcnn::check_launch("anchor_compact_kernel");
}

extern "C" int mrcnn_pyramid_patch_gather_f32(const float* const maps[8], const int32_t map_h[8], const int32_t map_w[8],
                                              int32_t levels, int32_t batch, int32_t channels, int32_t anchors_per_location,
                                              const int32_t* index, const int32_t* num, int32_t capacity, float* patches,
                                              mrcnn_stream_t stream) {
    const char* who = "pyramid_patch_gather";
    Pyramid p;
    if (int rc = fill_pyramid(who, p, const_cast<float* const*>(maps), false, map_h, map_w, levels, batch, channels,
                              anchors_per_location, capacity, index, num, patches))
        return rc;
    hipLaunchKernelGGL(patch_gather_kernel, dim3(static_cast<unsigned>(batch) * capacity), dim3(THREADS), 0, mrcnn::as_stream(stream),
                       p, channels / 4, capacity, index, num, reinterpret_cast<float4*>(patches));
    return mrcnn::check_launch("patch_gather_kernel");
}

extern "C" int mrcnn_pyramid_patch_scatter_f32(const float* dpatch, const int32_t map_h[8], const int32_t map_w[8], int32_t levels,
                                               int32_t batch, int32_t channels, int32_t anchors_per_location, const int32_t* index,
                                               const int32_t* num, int32_t capacity, float* const grad_maps[8],
                                               mrcnn_stream_t stream) {
    const char* who = "pyramid_patch_scatter";
    Pyramid p;
    if (int rc = fill_pyramid(who, p, grad_maps, true, map_h, map_w, levels, batch, channels, anchors_per_location, capacity, index,
                              num, dpatch))
        return rc;
    long long grid = 0;
    for (int l = 0; l < levels; ++l) {
        p.tile_first[l] = static_cast<int>(grid);
        if (p.map[l]) grid += 1LL * batch * p.h[l] * ((p.w[l] + STRIP - 1) / STRIP);
        MRCNN_REQUIRE(grid <= 0x7FFFFFFF, "%s: %lld strips exceed one grid", who, grid);
    }
    if (grid == 0) return MRCNN_OK;   // no gradient asked for
    // a level that is not asked for has no strips: the next level starts at the same workgroup and find_level passes over it
    hipLaunchKernelGGL(patch_scatter_kernel, dim3(static_cast<unsigned>(grid)), dim3(THREADS), 0, mrcnn::as_stream(stream), p,
                       channels / 4, capacity, index, num, reinterpret_cast<const float4*>(dpatch));
    return mrcnn::check_launch("patch_scatter_kernel");
}
