// COCO run-length encoding of 8-bit masks on the GPU (gfx950): rleEncode + rleToString + rleArea + rleToBbox of
// cocoapi/common/maskApi.c for n masks in one call, everything on the device, no atomics, no host synchronisation.
//
// A mask is row-major in memory and RLE is column-major (j = x*H + y), so the unit of work is a CELL: one column of one
// segment of rows. Cells ordered (x, segment) ARE the column-major order, so a scan over the cells of a mask gives every
// cell the index of its first run. A lane owns four adjacent columns of one segment and walks down the rows with one
// 32-bit load per row: the lanes of a wave read 256 contiguous bytes of each row.
//
//   1 rle_count_kernel   per cell: transitions, the last three transition positions, on pixels, y extent
//   2 rle_scan_kernel    per mask: exclusive scan of (transitions, last three positions) over the cells; the totals give
//                        num_runs, and the on-pixel counts / extents give area and bbox
//   3 rle_emit_kernel<false>  per cell: bytes of its runs in the compressed string (a run's string needs the counts of runs
//                        i and i-2, i.e. the three transition positions before it: those came through the scan)
//   4 rle_bytes_scan_kernel   per mask: exclusive scan of the byte counts -> string offsets and string_bytes
//   5 rle_emit_kernel<true>   per cell: writes counts and string characters
// Passes 3 and 5 skip lanes whose four cells hold no transition (the zero canvas around a pasted mask), so the mask is
// read once in full and twice more only where it has edges. A mask with more runs than `capacity` is left out of
// passes 3 - 5 altogether: its counts / strings rows are never touched.
#include "common.hpp"
#include "workgroup.hpp"

#include <algorithm>
#include <climits>

namespace {

constexpr int kCols = 4;            // adjacent columns per lane: one 32-bit load per row
constexpr int kBlock = 256;         // count / emit workgroup
constexpr int kScanThreads = 1024;  // one workgroup scans one mask
constexpr int kMaxDim = 16384;
#ifndef MRCNN_RLE_MIN_LANES
#define MRCNN_RLE_MIN_LANES 65536   // rows are cut into segments until a call has this many lanes
#endif

// How a call is cut into cells; a function of (n, H, W) only, so mrcnn_rle_workspace_bytes and the launch agree.
struct Plan {
    int groups;      // lanes across a row: ceil(W / 4)
    int nseg;        // segments of rows per column (more of them when n * W alone would leave the chip empty)
    int seg_rows;    // rows per segment
    int64_t cells;   // W * nseg, per mask
};

Plan make_plan(int n, int h, int w) {
    Plan p;
    p.groups = (w + kCols - 1) / kCols;
    const int64_t lanes = (int64_t)std::max(n, 1) * p.groups;
    const int want = (int)std::min<int64_t>((MRCNN_RLE_MIN_LANES + lanes - 1) / lanes, 64);
    const int most = std::min(64, (h + 31) / 32);   // a segment is at least 32 rows
    const int nseg = std::max(1, std::min(want, most));
    p.seg_rows = (h + nseg - 1) / nseg;
    p.nseg = (h + p.seg_rows - 1) / p.seg_rows;
    p.cells = (int64_t)w * p.nseg;
    return p;
}

// Scan element of a cell: x = transitions, (y, z, w) = the last three transition positions, most recent first; a
// position that does not exist is 0, which is also the virtual position before the first run (cnts = diff([0, P.., H*W])).
__device__ __forceinline__ int4 join(const int4 a, const int4 b) {   // a earlier, b later
    int4 r;
    r.x = a.x + b.x;
    if (b.x >= 3) {
        r.y = b.y; r.z = b.z; r.w = b.w;
    } else if (b.x == 2) {
        r.y = b.y; r.z = b.z; r.w = a.y;
    } else if (b.x == 1) {
        r.y = b.y; r.z = a.y; r.w = a.z;
    } else {
        r.y = a.y; r.z = a.z; r.w = a.w;
    }
    return r;
}

struct RleParams {
    const uint8_t* masks;
    int64_t image_stride, row_stride;
    int n, h, w, threshold, capacity;
    Plan plan;
    // workspace, [n][cells] each
    int4* run;       // per cell (transitions, last three positions)
    int4* pre;       // exclusive scan of run: (index of the cell's first run, the three positions before it)
    uint2* aux;      // per cell (on pixels, ymin | ymax << 16)
    int* cbytes;     // per cell string bytes
    int* boff;       // exclusive scan of cbytes
    // outputs
    int32_t* num_runs;
    uint32_t* counts;
    uint8_t* strings;
    int32_t* string_bytes;
    int32_t* areas;
    int32_t* bboxes;
};

__device__ __forceinline__ uint32_t load_cols(const uint8_t* p, int ncols) {
    uint32_t v = 0;
    if (ncols == kCols) {
        __builtin_memcpy(&v, p, 4);   // one dword load (global memory takes any alignment: a cropped view needs no copy)
    } else {
        for (int c = 0; c < ncols; ++c) v |= (uint32_t)p[c] << (8 * c);
    }
    return v;
}

// bit c = column c is on; the bytes of columns past the row's end are 0 and 0 > threshold never holds
__device__ __forceinline__ uint32_t on_bits(uint32_t v, int threshold) {
    uint32_t bits = 0;
#pragma unroll
    for (int c = 0; c < kCols; ++c) bits |= (uint32_t)((int)((v >> (8 * c)) & 255u) > threshold) << c;
    return bits;
}

// The lane's place in the call, and the value of the pixel that precedes each of its cells in column-major order.
struct Lane {
    int m, seg, x0, ncols, y0, y1;
    const uint8_t* img;
    uint32_t prev;
};

__device__ __forceinline__ bool lane_setup(const RleParams& p, Lane& l) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= p.plan.groups * p.plan.nseg) return false;
    l.m = blockIdx.y;
    l.seg = t / p.plan.groups;
    l.x0 = (t - l.seg * p.plan.groups) * kCols;
    l.ncols = min(kCols, p.w - l.x0);
    l.y0 = l.seg * p.plan.seg_rows;
    l.y1 = min(p.h, l.y0 + p.plan.seg_rows);
    l.img = p.masks + (int64_t)l.m * p.image_stride;
    l.prev = 0;
    for (int c = 0; c < l.ncols; ++c) {
        const int x = l.x0 + c;
        int v = 0;   // v(-1) = 0
        if (l.y0 > 0)
            v = l.img[(int64_t)(l.y0 - 1) * p.row_stride + x];
        else if (x > 0)
            v = l.img[(int64_t)(p.h - 1) * p.row_stride + x - 1];   // a run continues into the top of the next column
        l.prev |= (uint32_t)(v > p.threshold) << c;
    }
    return true;
}

// f(bits, y) for every row of the lane's segment whose four pixels are not all off-after-off; eight loads in flight.
template <class F>
__device__ __forceinline__ void walk_rows(const RleParams& p, const Lane& l, F&& f) {
    const uint8_t* q = l.img + (int64_t)l.y0 * p.row_stride + l.x0;
    uint32_t prev = l.prev;
    int y = l.y0;
    for (; y + 8 <= l.y1; y += 8) {
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = load_cols(q + (int64_t)k * p.row_stride, l.ncols);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t bits = on_bits(v[k], p.threshold);
            if ((bits | prev) != 0) f(bits, prev, y + k);
            prev = bits;
        }
        q += 8 * p.row_stride;
    }
    for (; y < l.y1; ++y) {
        const uint32_t bits = on_bits(load_cols(q, l.ncols), p.threshold);
        if ((bits | prev) != 0) f(bits, prev, y);
        prev = bits;
        q += p.row_stride;
    }
}

__global__ __launch_bounds__(kBlock) void rle_count_kernel(const RleParams p) {
    Lane l;
    if (!lane_setup(p, l)) return;
    int tc[kCols], p1[kCols], p2[kCols], p3[kCols], on[kCols], ymin[kCols], ymax[kCols];
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
        tc[c] = p1[c] = p2[c] = p3[c] = on[c] = ymax[c] = 0;
        ymin[c] = 0x7fff;
    }
    walk_rows(p, l, [&](uint32_t bits, uint32_t prev, int y) {
        const uint32_t changed = bits ^ prev;
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            if ((changed >> c) & 1u) {
                ++tc[c];
                p3[c] = p2[c];
                p2[c] = p1[c];
                p1[c] = (l.x0 + c) * p.h + y;   // < 2^28
            }
            if ((bits >> c) & 1u) {
                ++on[c];
                ymin[c] = min(ymin[c], y);
                ymax[c] = y;
            }
        }
    });
    const int64_t base = (int64_t)l.m * p.plan.cells + (int64_t)l.x0 * p.plan.nseg + l.seg;
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
        if (c < l.ncols) {
            p.run[base + (int64_t)c * p.plan.nseg] = make_int4(tc[c], p1[c], p2[c], p3[c]);
            p.aux[base + (int64_t)c * p.plan.nseg] = make_uint2((uint32_t)on[c], (uint32_t)ymin[c] | ((uint32_t)ymax[c] << 16));
        }
    }
}

// One workgroup scans one mask's cells (chunked_exclusive_scan, workgroup.hpp); the extents and the area are reduced beside it.
__global__ __launch_bounds__(kScanThreads) void rle_scan_kernel(const RleParams p) {
    __shared__ int4 lds[2 * kScanThreads];
    __shared__ int red[kScanThreads / mrcnn::kWave];
    const int m = blockIdx.x;
    const int64_t base = (int64_t)m * p.plan.cells;
    const int4 total = mrcnn::chunked_exclusive_scan<kScanThreads>(p.run + base, p.pre + base, p.plan.cells, make_int4(0, 0, 0, 0),
                                                                   lds, [](const int4 a, const int4 b) { return join(a, b); });

    const int t = threadIdx.x;
    const int64_t chunk = (p.plan.cells + kScanThreads - 1) / kScanThreads;
    const int64_t lo = min((int64_t)t * chunk, p.plan.cells), hi = min(lo + chunk, p.plan.cells);
    int area = 0, xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
    for (int64_t i = lo; i < hi; ++i) {
        const uint2 a = p.aux[base + i];
        if (a.x) {
            const int x = (int)(i / p.plan.nseg);
            area += (int)a.x;   // <= 2^28 in all
            xmin = min(xmin, x);
            xmax = max(xmax, x);
            ymin = min(ymin, (int)(a.y & 0xffffu));
            ymax = max(ymax, (int)(a.y >> 16));
        }
    }
    auto fmin = [](int a, int b) { return min(a, b); };
    auto fmax = [](int a, int b) { return max(a, b); };
    area = mrcnn::block_reduce<kScanThreads>(area, red, [](int a, int b) { return a + b; });
    xmin = mrcnn::block_reduce<kScanThreads>(xmin, red, fmin);
    xmax = mrcnn::block_reduce<kScanThreads>(xmax, red, fmax);
    ymin = mrcnn::block_reduce<kScanThreads>(ymin, red, fmin);
    ymax = mrcnn::block_reduce<kScanThreads>(ymax, red, fmax);
    if (t == 0) {
        p.num_runs[m] = total.x + 1;
        p.areas[m] = area;
        int32_t* bb = p.bboxes + 4 * (int64_t)m;
        bb[0] = area ? xmin : 0;
        bb[1] = area ? ymin : 0;
        bb[2] = area ? xmax - xmin + 1 : 0;
        bb[3] = area ? ymax - ymin + 1 : 0;
    }
}

__global__ __launch_bounds__(kScanThreads) void rle_bytes_scan_kernel(const RleParams p) {
    __shared__ int lds[2 * kScanThreads];
    const int m = blockIdx.x;
    if (p.num_runs[m] > p.capacity) {   // overflow (the whole workgroup takes this branch)
        if (threadIdx.x == 0) p.string_bytes[m] = 0;
        return;
    }
    const int64_t base = (int64_t)m * p.plan.cells;
    const int total = mrcnn::chunked_exclusive_scan<kScanThreads>(p.cbytes + base, p.boff + base, p.plan.cells, 0, lds,
                                                                  [](int a, int b) { return a + b; });
    if (threadIdx.x == 0) p.string_bytes[m] = total;
}

template <bool WRITE>
__global__ __launch_bounds__(kBlock) void rle_emit_kernel(const RleParams p) {
    Lane l;
    if (!lane_setup(p, l)) return;
    if (p.num_runs[l.m] > p.capacity) return;   // overflow: this mask's rows are not written at all
    const int64_t base = (int64_t)l.m * p.plan.cells + (int64_t)l.x0 * p.plan.nseg + l.seg;
    // the closing run (up to H*W) belongs to the last cell of the mask
    const bool closes = l.seg == p.plan.nseg - 1 && l.x0 + l.ncols == p.w;
    bool any = closes;
#pragma unroll
    for (int c = 0; c < kCols; ++c)
        if (c < l.ncols) any |= p.run[base + (int64_t)c * p.plan.nseg].x != 0;
    if (!any) {
        if (!WRITE)
            for (int c = 0; c < l.ncols; ++c) p.cbytes[base + (int64_t)c * p.plan.nseg] = 0;
        return;
    }
    int idx[kCols], q1[kCols], q2[kCols], q3[kCols], bo[kCols];
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
        idx[c] = q1[c] = q2[c] = q3[c] = bo[c] = 0;
        if (c < l.ncols) {
            const int4 s = p.pre[base + (int64_t)c * p.plan.nseg];
            idx[c] = s.x; q1[c] = s.y; q2[c] = s.z; q3[c] = s.w;
            if (WRITE) bo[c] = p.boff[base + (int64_t)c * p.plan.nseg];
        }
    }
    uint32_t* counts = WRITE && p.counts ? p.counts + (int64_t)l.m * p.capacity : nullptr;
    uint8_t* str = WRITE && p.strings ? p.strings + (int64_t)l.m * 6 * p.capacity : nullptr;
    // run idx ends at position pos: cnts[idx] = pos - P[idx-1]; the string holds cnts[idx] - cnts[idx-2] from run 3 on
    auto run_ends = [&](int& i, int& a1, int& a2, int& a3, int& b, int pos) {
        const int cnt = pos - a1;
        const int x = cnt - (i > 2 ? a2 - a3 : 0);
        if (WRITE) {
            if (i < p.capacity) {   // always: num_runs <= capacity here
                if (counts) counts[i] = (uint32_t)cnt;
                if (str) b += mrcnn::rle_put_value<true>(str + b, x);   // up to 6 characters: |x| <= 2^28
            }
        } else {
            b += mrcnn::rle_put_value<false>(nullptr, x);
        }
        a3 = a2; a2 = a1; a1 = pos;
        ++i;
    };
    walk_rows(p, l, [&](uint32_t bits, uint32_t prev, int y) {
        const uint32_t changed = bits ^ prev;
#pragma unroll
        for (int c = 0; c < kCols; ++c)
            if ((changed >> c) & 1u) run_ends(idx[c], q1[c], q2[c], q3[c], bo[c], (l.x0 + c) * p.h + y);
    });
    if (closes) {
#pragma unroll
        for (int c = 0; c < kCols; ++c)
            if (c == l.ncols - 1) run_ends(idx[c], q1[c], q2[c], q3[c], bo[c], p.h * p.w);
    }
    if (!WRITE) {
#pragma unroll
        for (int c = 0; c < kCols; ++c)
            if (c < l.ncols) p.cbytes[base + (int64_t)c * p.plan.nseg] = bo[c];
    }
}

constexpr size_t kAlign = 256;
size_t aligned(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

bool dims_ok(int n, int h, int w) { return n >= 0 && n <= 65535 && h >= 1 && h <= kMaxDim && w >= 1 && w <= kMaxDim; }

}  // namespace

extern "C" size_t mrcnn_rle_workspace_bytes(int32_t n, int32_t height, int32_t width) {
    if (!dims_ok(n, height, width) || n == 0) return 0;
    const size_t cells = (size_t)n * (size_t)make_plan(n, height, width).cells;
    return 2 * aligned(cells * sizeof(int4)) + aligned(cells * sizeof(uint2)) + 2 * aligned(cells * sizeof(int));
}

extern "C" int mrcnn_rle_encode_u8(const uint8_t* masks, int64_t image_stride, int64_t row_stride, int32_t n, int32_t height,
                                   int32_t width, int32_t threshold, int32_t capacity, int32_t* num_runs, uint32_t* counts,
                                   uint8_t* strings, int32_t* string_bytes, int32_t* areas, int32_t* bboxes, void* workspace,
                                   size_t workspace_bytes, mrcnn_stream_t stream) {
    MRCNN_REQUIRE(dims_ok(n, height, width), "rle_encode: n=%d (0..65535), mask %dx%d (1..%d each)", n, height, width, kMaxDim);
    MRCNN_REQUIRE(threshold >= 0 && threshold <= 254, "rle_encode: threshold=%d must be in [0,254]", threshold);
    MRCNN_REQUIRE(capacity >= 1, "rle_encode: capacity=%d must be >= 1", capacity);
    MRCNN_REQUIRE(row_stride >= width, "rle_encode: row stride %lld is shorter than a row of %d pixels", (long long)row_stride,
                  width);
    if (n == 0) return MRCNN_OK;
    MRCNN_REQUIRE(masks && num_runs && string_bytes && areas && bboxes, "rle_encode: null pointer");
    const size_t need = mrcnn_rle_workspace_bytes(n, height, width);
    MRCNN_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                  "rle_encode: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, workspace_bytes);

    RleParams p;
    p.masks = masks; p.image_stride = image_stride; p.row_stride = row_stride;
    p.n = n; p.h = height; p.w = width; p.threshold = threshold; p.capacity = capacity;
    p.plan = make_plan(n, height, width);
    const size_t cells = (size_t)n * (size_t)p.plan.cells;
    char* ws = static_cast<char*>(workspace);
    p.run = reinterpret_cast<int4*>(ws);     ws += aligned(cells * sizeof(int4));
    p.pre = reinterpret_cast<int4*>(ws);     ws += aligned(cells * sizeof(int4));
    p.aux = reinterpret_cast<uint2*>(ws);    ws += aligned(cells * sizeof(uint2));
    p.cbytes = reinterpret_cast<int*>(ws);   ws += aligned(cells * sizeof(int));
    p.boff = reinterpret_cast<int*>(ws);
    p.num_runs = num_runs; p.counts = counts; p.strings = strings; p.string_bytes = string_bytes;
    p.areas = areas; p.bboxes = bboxes;

    hipStream_t s = mrcnn::as_stream(stream);
    const dim3 grid((p.plan.groups * p.plan.nseg + kBlock - 1) / kBlock, n);
    hipLaunchKernelGGL(rle_count_kernel, grid, dim3(kBlock), 0, s, p);
    hipLaunchKernelGGL(rle_scan_kernel, dim3(n), dim3(kScanThreads), 0, s, p);
    hipLaunchKernelGGL(rle_emit_kernel<false>, grid, dim3(kBlock), 0, s, p);
    hipLaunchKernelGGL(rle_bytes_scan_kernel, dim3(n), dim3(kScanThreads), 0, s, p);
    if (counts || strings) hipLaunchKernelGGL(rle_emit_kernel<true>, grid, dim3(kBlock), 0, s, p);
    return mrcnn::check_launch("rle_encode");
}
