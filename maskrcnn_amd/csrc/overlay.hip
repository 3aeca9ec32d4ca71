// Rendering detections onto the image: data.blend_image / data.blend_mask (data.py:346-403) without the labels, ONE launch.
//
// Per pixel the reference's PIL calls (Image.blend at 0.2, two Image.composite, ImageFilter.CONTOUR inverted with the frame
// zeroed, ImageDraw.rectangle at width 1) reduce to: for instance i = 0 .. n-1 in order,
//   mask_i on at p      → px = (uint8) trunc(float(px) + 0.2f * float(int(c_i) - int(px)))   per channel, fp32, no FMA
//   else                → px = c_i where one of p's 8 neighbours is on in mask_i and p is not on the image frame
// then the rectangles in order (rows y0 and y1 over x0..x1, columns x0 and x1 over min(y0+1, y1)..max(y0+1, y1), clipped).
// Nothing a pixel needs depends on another pixel's result, so a lane owns kRun = 16 consecutive pixels of one row and keeps their
// 48 channel values in registers (as floats: every value is an integer 0..255, exact in fp32, so int(c) - int(px) is the fp32
// difference) across the whole instance loop and the rectangle loop.
//
// Per instance a lane reads the three mask rows y-1, y, y+1 over its run as 16-byte vectors; the halo byte on each side is the
// neighbouring lane's own (a DPP row shift: a tile row is 16 lanes), and only the lanes at a tile row's two ends load theirs.
// "Any byte > threshold" is tested on the packed dwords (two 16-bit lanes per dword: b + 255 - threshold carries into bit 8),
// and only when its 3 x 18 window has an on pixel does a lane turn the rows into 18-bit masks; on / neighbour / outline are
// shifts and ORs of those. A workgroup is 16 lanes x 16 rows = a 256 x 16 pixel tile, so of the 18 mask rows it reads 16 are its
// own and the two halo rows are its vertical neighbours' (L2). Colours and boxes are staged through LDS kChunk instances at a time.
//
// The 16-byte loads and stores need 16-byte-aligned bases and strides (vec_mask for the masks, vec_image for image and out,
// decided on the host). A wave takes the masks' 16-byte path when every one of its lanes has its whole run inside the width;
// the waves of a ragged last tile column, and every wave of an unaligned operand, go byte by byte: the same bits. The 16-byte
// path's loads are unconditional from clamped addresses and kAhead instances deep, so a lane waits for memory once per kAhead
// instances, not once per load.
// No atomics, no workspace, no host synchronisation; the same bits from run to run.
#include "common.hpp"

namespace {

constexpr int kRun = 16;                 // pixels of one row per lane
constexpr int kLanesX = 16;              // lanes across a tile row
constexpr int kRows = 16;                // rows of a tile
constexpr int kBlock = kLanesX * kRows;  // 256 threads: a 256 x 16 pixel tile
constexpr int kChunk = kBlock;           // instances whose colours / boxes are in LDS at a time
constexpr int kAhead = 4;                // instances whose mask rows a lane has in flight
constexpr int kMaxDim = 16384;
constexpr int kMaxInstances = 65535;

struct BlendParams {
    const uint8_t* image;
    const uint8_t* masks;
    const uint8_t* colors;
    const int32_t* boxes;
    uint8_t* out;
    int64_t image_row_stride, mask_image_stride, mask_row_stride, out_row_stride;
    int32_t n, h, w;
    uint32_t ge_add;   // (256 - (threshold + 1)) in both 16-bit halves: adding it to a byte sets bit 8 iff byte > threshold
    int32_t threshold;
    int32_t vec_mask, vec_image;
};

// bit 8 or bit 24 is set iff one of the dword's four bytes is > threshold
__device__ __forceinline__ uint32_t any_over(uint32_t v, uint32_t ge_add) {
    return ((v & 0x00ff00ffu) + ge_add) | (((v >> 8) & 0x00ff00ffu) + ge_add);
}

// bit j = (byte j of v > threshold), j = 0..3
__device__ __forceinline__ uint32_t bits4(uint32_t v, uint32_t ge_add) {
    const uint32_t g = ((((v & 0x00ff00ffu) + ge_add) >> 8) & 0x00010001u) | ((((v >> 8) & 0x00ff00ffu) + ge_add) & 0x01000100u);
    return (g | (g >> 7) | (g >> 14) | (g >> 21)) & 0xfu;   // flags at bits 0, 8, 16, 24 → bits 0..3
}

// One mask row over a lane's run with its halo: bit 0 = column x0-1, bits 1..16 = the run, bit 17 = column x0+16.
struct MaskRow {
    uint4 v;
    uint32_t left, right;
};

// `row` is a valid row of the mask.
// kVec — the run lies inside the row and row + x0 is 16-byte aligned: three unconditional loads, the halo bytes from clamped
// addresses, NOTHING zeroed. A row above or below the image is given as row y itself and a halo column outside the row as the
// row's first or last pixel: what lies outside the image counts as off, but it is a neighbour of frame pixels only (y = 0,
// y = h-1, x = 0, x = w-1), which never get an outline, and `on` is the centre row's own bits — so the duplicate changes no
// pixel. It matters that nothing is selected: hipcc sinks a load whose value is only used under a condition into a branch and
// waits for it at the branch's end, one memory latency per load; as they are, kAhead instances' loads are in flight together.
// The byte path loads under its bounds checks, one after the other (`live`: the row is inside the image): unconditional, its
// 54 loads per instance with an address pair each would set the register allocation of the whole kernel.
template <bool kVec>
__device__ __forceinline__ MaskRow load_mask_row(const uint8_t* row, bool live, int x0, int w) {
    MaskRow r;
    if (kVec) {
        r.v = *reinterpret_cast<const uint4*>(row + x0);
        r.left = r.right = 0u;                            // blend_chunk fills them in from the neighbouring lanes
    } else {
        uint32_t d[4] = {0u, 0u, 0u, 0u};
        r.left = r.right = 0u;
        if (live) {
#pragma unroll
            for (int j = 0; j < kRun; ++j)
                if (x0 + j < w) d[j >> 2] |= (uint32_t)row[x0 + j] << (8 * (j & 3));
            if (x0 > 0) r.left = row[x0 - 1];
            if (x0 + kRun < w) r.right = row[x0 + kRun];
        }
        r.v = make_uint4(d[0], d[1], d[2], d[3]);
    }
    return r;
}

__device__ __forceinline__ uint32_t row_any(const MaskRow& r, uint32_t ge_add) {
    return any_over(r.v.x, ge_add) | any_over(r.v.y, ge_add) | any_over(r.v.z, ge_add) | any_over(r.v.w, ge_add) |
           any_over(r.left | (r.right << 16), ge_add);
}

__device__ __forceinline__ uint32_t row_bits(const MaskRow& r, uint32_t ge_add, int threshold) {
    const uint32_t run = bits4(r.v.x, ge_add) | (bits4(r.v.y, ge_add) << 4) | (bits4(r.v.z, ge_add) << 8) | (bits4(r.v.w, ge_add) << 12);
    return ((int)r.left > threshold ? 1u : 0u) | (run << 1) | ((int)r.right > threshold ? 1u << 17 : 0u);
}

// One instance on a lane's run: px (48 channel values) is blended where the mask is on and set to the colour on the outline.
__device__ __forceinline__ void apply_instance(float (&px)[3 * kRun], const MaskRow& r0, const MaskRow& r1, const MaskRow& r2,
                                               const uint32_t* color_entry, uint32_t inner, uint32_t ge_add, int threshold) {
    if (((row_any(r0, ge_add) | row_any(r1, ge_add) | row_any(r2, ge_add)) & 0x01000100u) == 0u) return;
    const uint32_t b0 = row_bits(r0, ge_add, threshold);
    const uint32_t b1 = row_bits(r1, ge_add, threshold);
    const uint32_t b2 = row_bits(r2, ge_add, threshold);
    const uint32_t above_below = b0 | b2;
    const uint32_t near = above_below | (above_below << 1) | (above_below >> 1) | (b1 << 1) | (b1 >> 1);
    const uint32_t on = (b1 >> 1) & 0xffffu;
    const uint32_t edge = (near >> 1) & ~on & inner;
    if ((on | edge) == 0u) return;
    const uint32_t color = *color_entry;                 // LDS, read by the few lanes that get here
    const float cf[3] = {(float)(color & 0xffu), (float)((color >> 8) & 0xffu), (float)((color >> 16) & 0xffu)};
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
        if ((on >> j) & 1u) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float v = px[3 * j + ch];
                px[3 * j + ch] = truncf(v + 0.2f * (cf[ch] - v));    // cf - v is exact: both are integers 0..255
            }
        } else if ((edge >> j) & 1u) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) px[3 * j + ch] = cf[ch];
        }
    }
}

// `count` instances (their colours in s_color) on a lane's run, in order; m: the lane's row y of the first of them.
// kAhead instances' rows are requested before the first of them is looked at: a lane walks its instances in order, and one
// memory latency per instance is what the loop would otherwise cost.
template <bool kVec>
__device__ __forceinline__ void blend_chunk(float (&px)[3 * kRun], const BlendParams& p, const uint8_t* m, int count, int y, int x0,
                                            uint32_t inner, const uint32_t* s_color) {
    const bool up = y > 0, down = y + 1 < p.h;
    const int64_t above = up ? -p.mask_row_stride : 0, below = down ? p.mask_row_stride : 0;   // a row outside: row y
    constexpr int ahead = kVec ? kAhead : 1;
    // kVec: the halo byte a lane cannot get from a neighbouring lane — column x0-1 for the first lane of a tile row, column
    // x0+16 for the last lane of a tile row and for the last lane with pixels — comes from memory, clamped into the row (a
    // column outside the image is a neighbour of frame pixels only, see load_mask_row)
    const int lane16 = (int)threadIdx.x % kLanesX;
    const bool side_lane = lane16 == 0 || lane16 == kLanesX - 1 || x0 + 2 * kRun > p.w;
    const int side_x = lane16 == 0 ? max(x0 - 1, 0) : min(x0 + kRun, p.w - 1);
    uint32_t edge[ahead][3];
    for (int i0 = 0; i0 < count; i0 += ahead) {
        MaskRow rows[ahead][3];
#pragma unroll
        for (int k = 0; k < ahead; ++k) {
            const uint8_t* mk = m + (int64_t)min(i0 + k, count - 1) * p.mask_image_stride;   // past the end: the last one again
            rows[k][0] = load_mask_row<kVec>(mk + above, up, x0, p.w);
            rows[k][1] = load_mask_row<kVec>(mk, true, x0, p.w);
            rows[k][2] = load_mask_row<kVec>(mk + below, down, x0, p.w);
            if (kVec) {
#pragma unroll
                for (int r = 0; r < 3; ++r) edge[k][r] = 0u;
                if (side_lane) {                            // ONE branch for all of them: they are waited for once, at its end
                    edge[k][0] = mk[above + side_x];
                    edge[k][1] = mk[side_x];
                    edge[k][2] = mk[below + side_x];
                }
            }
        }
        if (kVec) {
            // The halo bytes are the neighbouring lanes' own: a tile row is 16 lanes, a DPP row. Lane i takes the last byte of
            // lane i-1 and the first byte of lane i+1; where there is no such lane in the row, or it has no pixels (its EXEC bit
            // is off), the DPP move keeps `old`: the byte the lane loaded itself, the side lanes' real halo.
#pragma unroll
            for (int k = 0; k < ahead; ++k)
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    rows[k][r].left = (uint32_t)__builtin_amdgcn_update_dpp((int)edge[k][r], (int)(rows[k][r].v.w >> 24), 0x111, 0xf, 0xf, false);
                    rows[k][r].right = (uint32_t)__builtin_amdgcn_update_dpp((int)edge[k][r], (int)(rows[k][r].v.x & 0xffu), 0x101, 0xf, 0xf, false);
                }
        }
#pragma unroll
        for (int k = 0; k < ahead; ++k)
            if (i0 + k < count)                             // uniform
                apply_instance(px, rows[k][0], rows[k][1], rows[k][2], &s_color[i0 + k], inner, p.ge_add, p.threshold);
    }
}

__global__ __launch_bounds__(kBlock) void blend_instances_kernel(BlendParams p) {
    __shared__ uint32_t s_color[kChunk];     // r | g << 8 | b << 16
    __shared__ int4 s_box[kChunk];           // (y0, x0, y1, x1)
    const int tid = (int)threadIdx.x;
    const int x0 = ((int)blockIdx.x * kLanesX + (tid % kLanesX)) * kRun;
    const int y = (int)blockIdx.y * kRows + tid / kLanesX;
    const bool active = x0 < p.w && y < p.h;          // an inactive lane only helps to stage colours and boxes
    const bool full = x0 + kRun <= p.w;

    float px[3 * kRun];
#pragma unroll
    for (int k = 0; k < 3 * kRun; ++k) px[k] = 0.f;
    if (active) {
        const uint8_t* src = p.image + (int64_t)y * p.image_row_stride + 3 * (int64_t)x0;
        if (p.vec_image && full) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = reinterpret_cast<const uint4*>(src)[q];
                const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; ++k) px[16 * q + k] = (float)((d[k >> 2] >> (8 * (k & 3))) & 0xffu);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3 * kRun; ++k)
                if (x0 + k / 3 < p.w) px[k] = (float)src[k];
        }
    }

    // columns of the run that exist and are not on the image frame, and whether this row is not
    uint32_t inner = 0u;
#pragma unroll
    for (int j = 0; j < kRun; ++j)
        if (x0 + j > 0 && x0 + j < p.w - 1) inner |= 1u << j;
    if (!(y > 0 && y < p.h - 1)) inner = 0u;

    const uint8_t* mrow = p.masks + (int64_t)y * p.mask_row_stride;

    for (int base = 0; base < p.n; base += kChunk) {
        const int count = min(kChunk, p.n - base);
        __syncthreads();                                   // the chunk before has been read by every lane
        if (tid < count) {
            const uint8_t* c = p.colors + 3 * (int64_t)(base + tid);
            s_color[tid] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
        }
        __syncthreads();
        if (active) {
            // the 16-byte loads when every lane of the wave that has pixels has its whole run inside the width: one uniform branch
            const bool whole_runs = __builtin_amdgcn_ballot_w64(!full) == 0;
            if (p.vec_mask && whole_runs)
                blend_chunk<true>(px, p, mrow + (int64_t)base * p.mask_image_stride, count, y, x0, inner, s_color);
            else
                blend_chunk<false>(px, p, mrow + (int64_t)base * p.mask_image_stride, count, y, x0, inner, s_color);
        }
    }

    // rectangles, in order: a later one overwrites an earlier one
    if (p.boxes != nullptr) {
        for (int base = 0; base < p.n; base += kChunk) {
            const int count = min(kChunk, p.n - base);
            __syncthreads();
            if (tid < count) {
                const int32_t* b = p.boxes + 4 * (int64_t)(base + tid);
                s_color[tid] = (uint32_t)p.colors[3 * (int64_t)(base + tid)] | ((uint32_t)p.colors[3 * (int64_t)(base + tid) + 1] << 8) |
                               ((uint32_t)p.colors[3 * (int64_t)(base + tid) + 2] << 16);
                s_box[tid] = make_int4(b[0], b[1], b[2], b[3]);
            }
            __syncthreads();
            for (int i = 0; active && i < count; ++i) {
                const int4 b = s_box[i];                      // x = y0, y = x0, z = y1, w = x1
                if (b.z < b.x || b.w < b.y) continue;         // an inverted box draws nothing
                const int lo = max(b.y, x0), hi = min(b.w, x0 + kRun - 1);   // the box's columns inside this run
                uint32_t bits = 0u;
                if ((y == b.x || y == b.z) && lo <= hi) bits = ((2u << (hi - x0)) - 1u) & ~((1u << (lo - x0)) - 1u);
                const int64_t y0p1 = (int64_t)b.x + 1;        // 64 bits: y0 may be INT32_MAX
                const int64_t vlo = y0p1 < b.z ? y0p1 : b.z, vhi = y0p1 < b.z ? (int64_t)b.z : y0p1;
                if (y >= vlo && y <= vhi) {
                    if (b.y >= x0 && b.y < x0 + kRun) bits |= 1u << (b.y - x0);
                    if (b.w >= x0 && b.w < x0 + kRun) bits |= 1u << (b.w - x0);
                }
                if (bits == 0u) continue;
                const uint32_t c = s_color[i];
                const float cf[3] = {(float)(c & 0xffu), (float)((c >> 8) & 0xffu), (float)((c >> 16) & 0xffu)};
#pragma unroll
                for (int j = 0; j < kRun; ++j)
                    if ((bits >> j) & 1u) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) px[3 * j + ch] = cf[ch];
                    }
            }
        }
    }

    if (!active) return;
    uint8_t* dst = p.out + (int64_t)y * p.out_row_stride + 3 * (int64_t)x0;
    if (p.vec_image && full) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            uint32_t d[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                d[k] = (uint32_t)px[16 * q + 4 * k] | ((uint32_t)px[16 * q + 4 * k + 1] << 8) | ((uint32_t)px[16 * q + 4 * k + 2] << 16) |
                       ((uint32_t)px[16 * q + 4 * k + 3] << 24);
            reinterpret_cast<uint4*>(dst)[q] = make_uint4(d[0], d[1], d[2], d[3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * kRun; ++k)
            if (x0 + k / 3 < p.w) dst[k] = (uint8_t)px[k];
    }
}

bool aligned16(const void* ptr, int64_t a, int64_t b = 0) { return ((reinterpret_cast<uintptr_t>(ptr) | (uint64_t)a | (uint64_t)b) & 15u) == 0; }

}  // namespace

extern "C" int mrcnn_blend_instances_u8(const uint8_t* image, int64_t image_row_stride, const uint8_t* masks,
                                        int64_t mask_image_stride, int64_t mask_row_stride, const uint8_t* colors,
                                        const int32_t* boxes, int32_t n, int32_t height, int32_t width, int32_t threshold,
                                        uint8_t* out, int64_t out_row_stride, mrcnn_stream_t stream) {
    MRCNN_REQUIRE(height >= 1 && height <= kMaxDim && width >= 1 && width <= kMaxDim, "blend_instances: image %dx%d (1..%d each)",
                  height, width, kMaxDim);
    MRCNN_REQUIRE(n >= 0 && n <= kMaxInstances, "blend_instances: n=%d must be in [0, %d]", n, kMaxInstances);
    MRCNN_REQUIRE(threshold >= 0 && threshold <= 254, "blend_instances: threshold=%d must be in [0, 254]", threshold);
    MRCNN_REQUIRE(image_row_stride >= 3 * (int64_t)width && out_row_stride >= 3 * (int64_t)width,
                  "blend_instances: image row stride %lld / out row stride %lld is shorter than a row of %d RGB pixels",
                  (long long)image_row_stride, (long long)out_row_stride, width);
    MRCNN_REQUIRE(mask_row_stride >= width, "blend_instances: mask row stride %lld is shorter than a row of %d pixels",
                  (long long)mask_row_stride, width);
    MRCNN_REQUIRE(mask_image_stride >= 0, "blend_instances: mask image stride %lld must be >= 0", (long long)mask_image_stride);
    MRCNN_REQUIRE(image && out && (n == 0 || (masks && colors)), "blend_instances: null pointer");
    BlendParams p;
    p.image = image; p.masks = masks; p.colors = colors; p.boxes = boxes; p.out = out;
    p.image_row_stride = image_row_stride; p.mask_image_stride = mask_image_stride; p.mask_row_stride = mask_row_stride;
    p.out_row_stride = out_row_stride;
    p.n = n; p.h = height; p.w = width; p.threshold = threshold;
    p.ge_add = (uint32_t)(255 - threshold) * 0x00010001u;
    p.vec_mask = n > 0 && aligned16(masks, mask_image_stride, mask_row_stride);
    p.vec_image = aligned16(image, image_row_stride) && aligned16(out, out_row_stride);
    const dim3 grid((unsigned)((width + kLanesX * kRun - 1) / (kLanesX * kRun)), (unsigned)((height + kRows - 1) / kRows));
    hipLaunchKernelGGL(blend_instances_kernel, grid, dim3(kBlock), 0, mrcnn::as_stream(stream), p);
    return mrcnn::check_launch("blend_instances");
}
