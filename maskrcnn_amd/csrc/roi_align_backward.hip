// Backward of the pyramid RoIAlign (csrc/crop.hip, roi_align_pyramid_nhwc) to the four FPN maps, channels-last, for gfx950.
// The rule (include/maskrcnn_hip.h, mrcnn_roi_align_pyramid_backward_f32): grad_fm[l][b,y,x,c] is the fp32 sum, from +0, of the
// terms crop_cpu_backward (crop_cpu.cpp:205-263) adds to that element, over the RoIs of level l and image b in ascending index,
// then bin row, bin column and the taps top-left, top-right, bottom-left, bottom-right; each term separately rounded (FP
// contraction off). That is the order of the reference's serial loop, level by level.
//
// MAP-stationary: a scatter (one thread per gradient element, four atomics: crop_backward_nchw) has no order; the same sum taken
// as a GATHER by the thread that owns the map element has whatever order that thread walks in, at no cost.
//   launch 1  one thread per RoI: level (crop_math.hpp's roi_level, the forward's), image or "contributes nothing", and the
//             integer footprint [min lo, max hi] of its inside samples on each axis, from the Sample tables' integers → workspace.
//   launch 2  one workgroup (8 waves) per (level, image, 8 x 8 tile of pixels). Every wave walks the image's records 64 at a time
//             and finds the RoIs whose footprint meets the tile by ballot; the hits go to an LDS list in index order (prefix of
//             the ballot: no atomic counter). Whenever the list holds a chunk of RoIs (64, fewer for pools over 16: the chunk's
//             Sample tables are bounded by 32 KiB of LDS) the workgroup builds the chunk's tables, from them per RoI and tile
//             row / column the run of bins on that row / column, and every wave takes its row of the tile, a lane 4 consecutive
//             channels (a float4; 256-channel steps as in the forward): for each listed
//             RoI, each bin row whose lo or hi is the pixel's y, each bin column whose lo or hi is its x, one 16-byte load of
//             grad_out and the taps that land on the pixel, in tap order, into registers. A pixel is stored once per chunk; the
//             next chunk, if there is one, starts from the stored value (a thread reads back its own store: exact). A tile no RoI
//             meets stores zeros. Every byte of the maps is written; nothing is zeroed beforehand.
// The list a wave builds depends on the records alone, so all the waves agree on every count without exchanging it.
#pragma clang fp contract(off)

#include "common.hpp"
#include "crop_math.hpp"

namespace {

using mrcnn_crop::Sample;
using mrcnn_crop::make_sample;
using mrcnn_crop::roi_level;

constexpr int TILE = 8;              // pixels per tile side
// 8 waves, one row of the tile each. The tiles of the small maps, met by the most RoIs, are the critical path, and more waves
// shorten it; every wave walks the records, which is what the light tiles pay for them. profiles/roi_align_backward_threads_ab.jsonl
// holds the microbenchmark's lines for 256 and 512 (`build.py --variant NAME --only roi_align_backward.hip -DMRCNN_RAB_THREADS=N`,
// then tools/roi_align_backward_microbench.py --label threads=N on that build).
#ifndef MRCNN_RAB_THREADS
#define MRCNN_RAB_THREADS 512
#endif
constexpr int THREADS = MRCNN_RAB_THREADS;
static_assert(THREADS % 64 == 0 && THREADS >= 64 && THREADS <= 1024, "whole waves");
constexpr int MAX_CHUNK = 64;        // RoIs per chunk (= the records a wave tests at a time)
constexpr int TABLE_SAMPLES = 2048;  // Samples of a chunk's tables: chunk x 2 x pool <= 2048 (32 KiB)

struct Record {   // 32 bytes per RoI, read as two int4
    int level;    // 0..3 for P2..P5; -1: the RoI contributes nothing
    int image;
    int ylo, yhi, xlo, xhi;   // footprint on the level's map, inclusive
    int pad0, pad1;
};

struct BackwardArgs {
    float* gfm[4];
    int h[4], w[4];
    int tiles_x[4];
    int first[4];   // workgroup index at which level l starts. P5 comes FIRST and P2 last: the small maps' tiles are met by the
                    // most RoIs and run longest, so they start at once and the many light tiles of P2 fill in behind them
};

__host__ __device__ inline int chunk_for(int pool) { return pool <= 16 ? MAX_CHUNK : (TABLE_SAMPLES / 2) / pool; }

// launch 1: grid = max(1, ceil(num_rois / 256))
__global__ __launch_bounds__(256) void roi_backward_records(
    BackwardArgs a, int batch, const float* __restrict__ rois, const int* __restrict__ roi_batch, int num_rois,
    int rois_per_image, const int* __restrict__ roi_counts, int pool, float image_area, Record* __restrict__ records) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= num_rois) return;
    Record rec;
    rec.level = -1;
    rec.image = -1;
    rec.ylo = rec.xlo = 0;
    rec.yhi = rec.xhi = -1;
    rec.pad0 = rec.pad1 = 0;
    const int img = roi_batch ? roi_batch[r] : r / rois_per_image;
    bool live = img >= 0 && img < batch;
    if (live && roi_counts) live = r - img * rois_per_image < roi_counts[img];
    if (live) {
        const float y1 = rois[r * 4 + 0], x1 = rois[r * 4 + 1];
        const float y2 = rois[r * 4 + 2], x2 = rois[r * 4 + 3];
        const int li = roi_level(y1, x1, y2, x2, image_area) - 2;
        const int H = a.h[li], W = a.w[li];
        int ylo = 0x7FFFFFFF, yhi = -0x7FFFFFFF - 1, xlo = 0x7FFFFFFF, xhi = -0x7FFFFFFF - 1;
        for (int t = 0; t < pool; ++t) {
            const Sample Y = make_sample(y1, y2, H, pool, t);
            if (Y.inside) { ylo = min(ylo, Y.lo); yhi = max(yhi, Y.hi); }
            const Sample X = make_sample(x1, x2, W, pool, t);
            if (X.inside) { xlo = min(xlo, X.lo); xhi = max(xhi, X.hi); }
        }
        if (ylo <= yhi && xlo <= xhi) {
            rec.level = li;
            rec.image = img;
            rec.ylo = ylo; rec.yhi = yhi; rec.xlo = xlo; rec.xhi = xhi;
        }
    }
    int4* dst = reinterpret_cast<int4*>(records + r);
    dst[0] = make_int4(rec.level, rec.image, rec.ylo, rec.yhi);
    dst[1] = make_int4(rec.xlo, rec.xhi, 0, 0);
}

__device__ __forceinline__ void add4(float4& acc, const float4& g, float wy, float wx) {
    // one term of crop_cpu.cpp:254-260: wx * (wy * g), both products rounded
    acc.x = acc.x + wx * (wy * g.x);
    acc.y = acc.y + wx * (wy * g.y);
    acc.z = acc.z + wx * (wy * g.z);
    acc.w = acc.w + wx * (wy * g.w);
}

// launch 2: grid = the tiles of all levels and images, block = 512. LDS: Sample[chunk][2][pool].
__global__ __launch_bounds__(THREADS) void roi_backward_tiles(
    BackwardArgs a, int depth, const float* __restrict__ grad_out, const float* __restrict__ rois,
    const Record* __restrict__ records, int num_rois, int rois_per_image, int by_index, int pool, int chunk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Sample* tables = reinterpret_cast<Sample*>(smem);
    __shared__ int list[2 * MAX_CHUNK];      // RoI indices waiting for their chunk, in index order
    __shared__ int2 runs[MAX_CHUNK * 2 * TILE];   // per RoI of the chunk, tile row (8) and tile column (8): first and last bin on it

    const int wg = blockIdx.x;
    const int li = wg >= a.first[0] ? 0 : wg >= a.first[1] ? 1 : wg >= a.first[2] ? 2 : 3;
    const int H = a.h[li], W = a.w[li], tiles_x = a.tiles_x[li];
    const int tiles = tiles_x * ((H + TILE - 1) / TILE);
    const int rem = wg - a.first[li];
    const int img = rem / tiles, tile = rem - img * tiles;
    const int ty0 = (tile / tiles_x) * TILE, tx0 = (tile % tiles_x) * TILE;
    const int ty1 = min(ty0 + TILE, H) - 1, tx1 = min(tx0 + TILE, W) - 1;
    float* gmap = a.gfm[li] + static_cast<int64_t>(img) * H * W * depth;

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the wave's number, as a scalar
    // the records of this image: a contiguous run of slots, or (roi_batch) all of them, filtered by the record's image
    const int64_t slot0 = static_cast<int64_t>(img) * rois_per_image;
    const int r_begin = by_index ? 0 : static_cast<int>(min(static_cast<int64_t>(num_rois), slot0));
    const int r_end = by_index ? num_rois : static_cast<int>(min(static_cast<int64_t>(num_rois), slot0 + rois_per_image));
    int count = 0;        // RoIs in the list; the same in every wave
    bool first = true;    // no chunk has stored the tile yet

    // One chunk: the first n entries of the list. Barriers: the list and the previous chunk's readers before the tables are
    // built; the tables before the runs are taken from them; the runs before the waves read them; the readers before the list is
    // shifted or the next chunk's tables are built.
    auto process = [&](int n) {
        __syncthreads();
        const int per = 2 * pool;
        for (int e = threadIdx.x; e < n * per; e += THREADS) {
            const int k = e / per, s = e - k * per;
            const int r = list[k];
            const float c1 = rois[r * 4 + (s < pool ? 0 : 1)], c2 = rois[r * 4 + (s < pool ? 2 : 3)];
            tables[e] = s < pool ? make_sample(c1, c2, H, pool, s) : make_sample(c1, c2, W, pool, s - pool);
        }
        __syncthreads();
        // per RoI and tile row / tile column: the first and the last bin whose lo or hi is that row / column (a sample moves one
        // way with its bin, so they are a run; the walk below tests every bin of the run again and relies on no such argument)
        for (int e = threadIdx.x; e < n * 2 * TILE; e += THREADS) {
            const int k = e / (2 * TILE), axis = (e / TILE) & 1, v = (axis ? tx0 : ty0) + (e & (TILE - 1));
            const Sample* s = tables + k * per + axis * pool;
            int lo_bin = pool, hi_bin = -1;
            for (int t = 0; t < pool; ++t) {
                const Sample S = s[t];
                if (S.inside && (S.lo == v || S.hi == v)) { lo_bin = min(lo_bin, t); hi_bin = t; }
            }
            runs[e] = make_int2(lo_bin, hi_bin);
        }
        __syncthreads();
        for (int px = wave; px < TILE * TILE; px += THREADS / 64) {
            const int y = ty0 + px % TILE, x = tx0 + px / TILE;   // px = wave + 8 k: the wave's own row, column k
            if (y > ty1 || x > tx1) continue;
            float* o = gmap + (static_cast<int64_t>(y) * W + x) * depth;
            for (int c = lane * 4; c < depth; c += 256) {
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!first) acc = *reinterpret_cast<const float4*>(o + c);
                for (int k = 0; k < n; ++k) {
                    const int2 rows = runs[k * 2 * TILE + px % TILE], cols = runs[k * 2 * TILE + TILE + px / TILE];
                    if (rows.y < rows.x || cols.y < cols.x) continue;
                    const Sample* sy = tables + k * per;
                    const Sample* sx = sy + pool;
                    const float* g = grad_out + static_cast<int64_t>(list[k]) * pool * pool * depth + c;
                    for (int i = rows.x; i <= rows.y; ++i) {
                        const Sample Y = sy[i];
                        const bool top = Y.lo == y, bot = Y.hi == y;
                        if (!Y.inside || !(top || bot)) continue;
                        const float omy = 1.0f - Y.lerp;
                        for (int j = cols.x; j <= cols.y; ++j) {
                            const Sample X = sx[j];
                            const bool left = X.lo == x, right = X.hi == x;
                            if (!X.inside || !(left || right)) continue;
                            const float4 gv = *reinterpret_cast<const float4*>(g + (static_cast<int64_t>(i) * pool + j) * depth);
                            const float omx = 1.0f - X.lerp;
                            if (top && left) add4(acc, gv, omy, omx);
                            if (top && right) add4(acc, gv, omy, X.lerp);
                            if (bot && left) add4(acc, gv, Y.lerp, omx);
                            if (bot && right) add4(acc, gv, Y.lerp, X.lerp);
                        }
                    }
                }
                *reinterpret_cast<float4*>(o + c) = acc;
            }
        }
        __syncthreads();
        first = false;
    };

    for (int base = r_begin; base < r_end; base += 64) {
        const int r = base + lane;
        bool hit = false;
        if (r < r_end) {
            const int4* rec = reinterpret_cast<const int4*>(records + r);
            const int4 p = rec[0];   // level, image, ylo, yhi
            if (p.x == li && p.y == img && p.z <= ty1 && p.w >= ty0) {
                const int4 q = rec[1];   // xlo, xhi
                hit = q.x <= tx1 && q.y >= tx0;
            }
        }
        const unsigned long long mask = __ballot(hit);
        if (wave == 0 && hit) list[count + __popcll(mask & ((1ull << lane) - 1ull))] = r;
        count += __popcll(mask);
        while (count >= chunk) {
            process(chunk);
            // wave 0 alone moves the rest (fewer than 64 entries) to the front: one read and one write per lane, in that order
            if (wave == 0) {
                const int rest = count - chunk;
                const int v = lane < rest ? list[chunk + lane] : 0;
                if (lane < rest) list[lane] = v;
            }
            count -= chunk;
        }
    }
    if (count > 0) process(count);
    if (first) {   // no RoI meets the tile
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int px = wave; px < TILE * TILE; px += THREADS / 64) {
            const int y = ty0 + px % TILE, x = tx0 + px / TILE;   // px = wave + 8 k: the wave's own row, column k
            if (y > ty1 || x > tx1) continue;
            float* o = gmap + (static_cast<int64_t>(y) * W + x) * depth;
            for (int c = lane * 4; c < depth; c += 256) *reinterpret_cast<float4*>(o + c) = zero;
        }
    }
}

}  // namespace

extern "C" size_t mrcnn_roi_align_pyramid_backward_workspace_bytes(int32_t num_rois) {
    return sizeof(Record) * static_cast<size_t>(num_rois > 0 ? num_rois : 0);
}

extern "C" int mrcnn_roi_align_pyramid_backward_f32(const float* grad_out, const int32_t fm_h[4], const int32_t fm_w[4],
                                                    int32_t batch, int32_t depth, const float* rois, const int32_t* roi_batch,
                                                    int32_t num_rois, int32_t rois_per_image, const int32_t* roi_counts,
                                                    int32_t pool, float image_area, float* const grad_fm[4], void* workspace,
                                                    size_t workspace_bytes, mrcnn_stream_t stream) {
    const char* who = "roi_align_pyramid_backward";
    MRCNN_REQUIRE(roi_counts == nullptr || (roi_batch == nullptr && rois_per_image >= 1 && num_rois % rois_per_image == 0),
                  "%s: roi_counts needs rois_per_image (no roi_batch) and whole images of slots", who);
    MRCNN_REQUIRE(fm_h && fm_w && grad_fm, "%s: null pointer", who);
    MRCNN_REQUIRE(batch >= 1, "%s: batch=%d must be at least 1", who, batch);
    MRCNN_REQUIRE(depth >= 4 && depth % 4 == 0, "%s: depth=%d must be a multiple of 4", who, depth);
    MRCNN_REQUIRE(pool >= 1 && pool <= 1024, "%s: pool=%d", who, pool);
    MRCNN_REQUIRE(roi_batch || rois_per_image >= 1, "%s: need roi_batch or rois_per_image", who);
    MRCNN_REQUIRE(num_rois >= 0, "%s: num_rois=%d", who, num_rois);
    MRCNN_REQUIRE(num_rois == 0 || (grad_out && rois), "%s: null pointer", who);
    const size_t need = mrcnn_roi_align_pyramid_backward_workspace_bytes(num_rois);
    MRCNN_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0),
                  "%s: workspace of %zu bytes (16-byte aligned) needed, got %zu", who, need, workspace_bytes);
    BackwardArgs a;
    int64_t grid = 0;
    for (int l = 3; l >= 0; --l) {
        MRCNN_REQUIRE(grad_fm[l] && fm_h[l] >= 1 && fm_w[l] >= 1, "%s: bad level %d", who, l);
        MRCNN_REQUIRE((reinterpret_cast<uintptr_t>(grad_fm[l]) & 15) == 0, "%s: grad_fm[%d] must be 16-byte aligned", who, l);
        a.gfm[l] = grad_fm[l];
        a.h[l] = fm_h[l];
        a.w[l] = fm_w[l];
        a.tiles_x[l] = (fm_w[l] + TILE - 1) / TILE;
        a.first[l] = static_cast<int>(grid);
        grid += static_cast<int64_t>(batch) * a.tiles_x[l] * ((fm_h[l] + TILE - 1) / TILE);
        MRCNN_REQUIRE(grid <= 0x7FFFFFFF, "%s: %lld tiles exceed one grid", who, static_cast<long long>(grid));
    }
    MRCNN_REQUIRE(num_rois == 0 || (reinterpret_cast<uintptr_t>(grad_out) & 15) == 0, "%s: grad_out must be 16-byte aligned", who);
    hipStream_t s = mrcnn::as_stream(stream);
    Record* records = static_cast<Record*>(workspace);
    // always two launches (num_rois == 0: one workgroup whose threads all leave at once)
    hipLaunchKernelGGL(roi_backward_records, dim3(std::max(1, (num_rois + 255) / 256)), dim3(256), 0, s, a, batch, rois, roi_batch,
                       num_rois, rois_per_image, roi_counts, pool, image_area, records);
    if (int rc = mrcnn::check_launch("roi_backward_records")) return rc;
    const int chunk = chunk_for(pool);
    const size_t lds = sizeof(Sample) * static_cast<size_t>(chunk) * 2 * pool;
    hipLaunchKernelGGL(roi_backward_tiles, dim3(static_cast<unsigned>(grid)), dim3(THREADS), lds, s, a, depth, grad_out, rois,
                       records, num_rois, rois_per_image, roi_batch ? 1 : 0, pool, chunk);
    return mrcnn::check_launch("roi_backward_tiles");
}
