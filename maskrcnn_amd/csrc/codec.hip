// The rest of the COCO RLE codec on the GPU (gfx950), applied to run-list TABLES (num_runs int32 [n], counts uint32 [n][capacity],
// off run first — what rle.hip and poly.hip write): rleFrString, rleToString, rleArea + rleToBbox and rleDecode of
// cocoapi/common/maskApi.c:218-231, :204-216, :72-75 + :133-147, :43-47, grouped, the reference's bits. No allocation, no host
// synchronisation, no atomics, the same bits from run to run. Integer work only.
//
// mrcnn_rle_from_string, a wave per string, 64 characters per step:
//   a token ends at a character whose (c - 48) & 0x20 is 0; the ballot of the end lanes gives every token its index (a popcount
//   of the ballot below the lane) and its first character (the end before it, or the one carried from the step before). The end
//   lane gathers its at most 6 characters. cnts[m] = x[m] + cnts[m-2] for m > 2 is two independent prefix sums — odd m from 1,
//   even m from 2, cnts[0] alone — so two wave scans per step, one per parity, each with a carry across the steps.
//   The string is swept twice: once to validate and count (a row with more runs than capacity is never written), once to write.
// mrcnn_rle_area_bbox, a wave per row: one scan of the counts gives cc; t, y, x and the min / max follow per lane.
// mrcnn_rle_to_string: pass 1 (a wave per row) sums the characters per row, one workgroup scans them into str_off
//   (chunked_exclusive_scan, workgroup.hpp), pass 2 (a wave per row) scans the characters per run within the row and writes them.
// mrcnn_rle_decode_u8: the encoder's transposition in reverse. A wave per row scans the counts to end positions (clipped at
//   H*W). Then a lane owns FOUR adjacent columns of a 32-row segment: one binary search per column finds the run its first pixel
//   lies in, then it walks down the rows and stores one 32-bit word per row — the lanes of a wave write 256 contiguous bytes of
//   each row, so the stores are contiguous along x without a trip through LDS.
#include "common.hpp"
#include "workgroup.hpp"

#include <climits>

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / mrcnn::kWave;
constexpr int kScanThreads = 1024;
constexpr int kMaxDim = 16384;
constexpr int kMaxRows = 1 << 24;     // strings / rows of one call
constexpr int kMaxToken = 6;          // characters: the reference's int shift is defined up to here
constexpr int kCols = 4;              // decode: adjacent columns per lane
constexpr int kSegRows = 32;          // decode: rows per lane
constexpr size_t kAlign = 256;
size_t aligned(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

enum : int32_t {
    kBadByte = 1, kLongToken = 2, kOpenToken = 4, kBadSize = 8, kEmptyRun = 16, kPixelSum = 32, kBadOffsets = 64,
};

using mrcnn::rle_put_value;
using mrcnn::wave_inclusive_scan;
using mrcnn::wave_reduce;

__device__ __forceinline__ bool row_ok(int nr, int capacity) { return nr >= 0 && nr <= capacity; }

// ------------------------------------------------------------------------------------------------ rleFrString
struct FromStringParams {
    const uint8_t* bytes;
    const int64_t* str_off;
    int64_t total;
    const int32_t* heights;
    const int32_t* widths;
    int32_t n, capacity;
    int32_t* num_runs;
    uint32_t* counts;
    int32_t* status;
};

__global__ __launch_bounds__(kBlock) void rle_from_string_kernel(const FromStringParams p) {
    const int lane = threadIdx.x & (mrcnn::kWave - 1);
    const int i = blockIdx.x * kWaves + threadIdx.x / mrcnn::kWave;   // wave-uniform
    if (i >= p.n) return;
    const int64_t s0 = p.str_off[i], s1 = p.str_off[i + 1];
    const int h = p.heights[i], w = p.widths[i];
    int32_t st = 0;
    if (h < 1 || h > kMaxDim || w < 1 || w > kMaxDim) st |= kBadSize;
    if (s0 < 0 || s1 < s0 || s1 > p.total || s1 - s0 > (int64_t)INT_MAX) st |= kBadOffsets;
    if (st & kBadOffsets) {
        if (lane == 0) {
            p.num_runs[i] = -1;
            p.status[i] = st;
        }
        return;
    }
    const uint8_t* s = p.bytes + s0;
    const int len = (int)(s1 - s0);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;

    // sweep 1: validate, count the tokens
    int count = 0, last_end = -1;
    bool bad_byte = false, long_token = false;
    for (int base = 0; base < len; base += mrcnn::kWave) {
        const int pos = base + lane;
        const int c = pos < len ? (int)s[pos] : 48 + 0x20;
        const bool bad = c < 48 || c > 111;
        const bool end = pos < len && !bad && !((c - 48) & 0x20);
        const unsigned long long ends = __ballot(end);
        bad_byte |= bad;
        if (end) {
            const unsigned long long before = ends & below;
            const int prev = before ? base + 63 - __clzll((long long)before) : last_end;
            long_token |= pos - prev > kMaxToken;
        }
        count += __popcll(ends);
        if (ends) last_end = base + 63 - __clzll((long long)ends);
    }
    if (__ballot(bad_byte)) st |= kBadByte;
    if (__ballot(long_token)) st |= kLongToken;
    if (last_end != len - 1) st |= kOpenToken;   // the string ends inside a token (a 7th continuation character is a long token too)
    if (st) {
        if (lane == 0) {
            p.num_runs[i] = -1;
            p.status[i] = st;
        }
        return;
    }
    if (count > p.capacity) {   // the true count; the row is not written
        if (lane == 0) {
            p.num_runs[i] = count;
            p.status[i] = 0;
        }
        return;
    }

    // sweep 2: values, the two parity chains, the checks on the runs
    uint32_t* row = p.counts + (int64_t)i * p.capacity;
    uint32_t carry_odd = 0, carry_even = 0;
    unsigned long long sum = 0;
    bool empty = false;
    int m0 = 0;
    last_end = -1;
    for (int base = 0; base < len; base += mrcnn::kWave) {
        const int pos = base + lane;
        const int c = pos < len ? (int)s[pos] - 48 : 0x20;
        const bool end = !(c & 0x20);
        const unsigned long long ends = __ballot(end);
        uint32_t x = 0;
        int m = 0;
        if (end) {
            const unsigned long long before = ends & below;
            const int prev = before ? base + 63 - __clzll((long long)before) : last_end;
            const int k = pos - prev;   // 1 .. 6
            m = m0 + __popcll(before);
            for (int j = 0; j < k; ++j) x |= ((uint32_t)(s[prev + 1 + j] - 48) & 0x1fu) << (5 * j);
            if (c & 0x10) x |= 0xffffffffu << (5 * k);
        }
        const bool odd = end && (m & 1), even = end && !(m & 1) && m > 0;
        const uint32_t so = wave_inclusive_scan(odd ? x : 0u, lane), se = wave_inclusive_scan(even ? x : 0u, lane);
        if (end) {
            const uint32_t v = odd ? carry_odd + so : even ? carry_even + se : x;
            row[m] = v;
            sum += v;
            empty |= m > 0 && v == 0;
        }
        carry_odd += __shfl(so, mrcnn::kWave - 1);
        carry_even += __shfl(se, mrcnn::kWave - 1);
        m0 += __popcll(ends);
        if (ends) last_end = base + 63 - __clzll((long long)ends);
    }
    sum = wave_reduce(sum, [](unsigned long long a, unsigned long long b) { return a + b; });
    if (__ballot(empty)) st |= kEmptyRun;
    if (sum != (unsigned long long)((long long)h * w)) st |= kPixelSum;
    if (lane == 0) {
        p.num_runs[i] = count;
        p.status[i] = st;
    }
}

// ------------------------------------------------------------------------------------------------ rleArea + rleToBbox
struct AreaParams {
    const int32_t* num_runs;
    const uint32_t* counts;
    const int32_t* heights;
    const int32_t* widths;
    int32_t n, capacity;
    int32_t* areas;
    int32_t* bboxes;
};

__global__ __launch_bounds__(kBlock) void rle_area_bbox_kernel(const AreaParams p) {
    const int lane = threadIdx.x & (mrcnn::kWave - 1);
    const int i = blockIdx.x * kWaves + threadIdx.x / mrcnn::kWave;
    if (i >= p.n) return;
    const int nr = p.num_runs[i];
    const int hi = p.heights[i], wi = p.widths[i];
    int32_t* bb = p.bboxes + 4 * (int64_t)i;
    if (!row_ok(nr, p.capacity) || hi < 1 || hi > kMaxDim || wi < 1 || wi > kMaxDim) {
        if (lane == 0) p.areas[i] = -1;
        if (lane < 4) bb[lane] = -1;
        return;
    }
    const uint32_t h = (uint32_t)hi, w = (uint32_t)wi;
    const uint32_t* row = p.counts + (int64_t)i * p.capacity;
    const int m = (nr / 2) * 2;
    uint32_t area = 0, cc = 0, xs = w, ys = h, xe = 0, ye = 0;
    bool cross = false;
    for (int base = 0; base < nr; base += mrcnn::kWave) {
        const int j = base + lane;
        const uint32_t c = j < nr ? row[j] : 0u;
        if (j & 1) area += c;   // j < nr, or c == 0
        const uint32_t e = cc + wave_inclusive_scan(j < m ? c : 0u, lane);
        const uint32_t t = e - (uint32_t)(j & 1), y = t % h, x = (t - y) / h;
        const uint32_t xp = __shfl_up(x, 1);   // an odd j sits in an odd lane: its even predecessor is in this step
        if (j < m) {
            if ((j & 1) && xp < x) cross = true;
            xs = min(xs, x); xe = max(xe, x); ys = min(ys, y); ye = max(ye, y);
        }
        cc = __shfl(e, mrcnn::kWave - 1);
    }
    auto fmin = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    auto fmax = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    area = wave_reduce(area, [](uint32_t a, uint32_t b) { return a + b; });
    xs = wave_reduce(xs, fmin); ys = wave_reduce(ys, fmin);
    xe = wave_reduce(xe, fmax); ye = wave_reduce(ye, fmax);
    if (__ballot(cross)) {
        ys = 0;
        ye = h - 1;
    }
    if (lane == 0) {
        p.areas[i] = (int32_t)area;
        bb[0] = m ? (int32_t)xs : 0;
        bb[1] = m ? (int32_t)ys : 0;
        bb[2] = m ? (int32_t)(xe - xs + 1) : 0;
        bb[3] = m ? (int32_t)(ye - ys + 1) : 0;
    }
}

// ------------------------------------------------------------------------------------------------ rleToString
struct ToStringParams {
    const int32_t* num_runs;
    const uint32_t* counts;
    int32_t n, capacity;
    uint8_t* bytes;
    int64_t bytes_capacity;
    int64_t* str_off;     // [n+1]
    int64_t* row_bytes;   // [n] workspace
    int64_t row_stride;   // 0: packed at str_off; > 0: row i at bytes + i*row_stride (rows longer than the stride are not written)
};

__device__ __forceinline__ long long string_value(const uint32_t* row, int j) {
    long long x = (long long)row[j];
    if (j > 2) x -= (long long)row[j - 2];
    return x;
}

__global__ __launch_bounds__(kBlock) void rle_string_bytes_kernel(const ToStringParams p) {
    const int lane = threadIdx.x & (mrcnn::kWave - 1);
    const int i = blockIdx.x * kWaves + threadIdx.x / mrcnn::kWave;
    if (i >= p.n) return;
    const int nr = p.num_runs[i];
    long long total = 0;
    if (row_ok(nr, p.capacity)) {
        const uint32_t* row = p.counts + (int64_t)i * p.capacity;
        for (int j = lane; j < nr; j += mrcnn::kWave) total += rle_put_value<false>(nullptr, string_value(row, j));
        total = wave_reduce(total, [](long long a, long long b) { return a + b; });
    }
    if (lane == 0) p.row_bytes[i] = total;
}

// exclusive scan of row_bytes into str_off[0..n], one workgroup
__global__ __launch_bounds__(kScanThreads) void rle_string_scan_kernel(const ToStringParams p) {
    __shared__ int64_t lds[2 * kScanThreads];
    const int64_t total = mrcnn::chunked_exclusive_scan<kScanThreads>(p.row_bytes, p.str_off, (int64_t)p.n, (int64_t)0, lds,
                                                                      [](int64_t a, int64_t b) { return a + b; });
    if (threadIdx.x == kScanThreads - 1) p.str_off[p.n] = total;   // the last thread: its chunk is the short one
}

__global__ __launch_bounds__(kBlock) void rle_string_write_kernel(const ToStringParams p) {
    const int lane = threadIdx.x & (mrcnn::kWave - 1);
    const int i = blockIdx.x * kWaves + threadIdx.x / mrcnn::kWave;
    if (i >= p.n) return;
    const int nr = p.num_runs[i];
    if (!row_ok(nr, p.capacity)) return;
    int64_t b0 = p.str_off[i], b1 = p.str_off[i + 1];
    if (p.row_stride > 0) {   // the fixed-stride layout: the row's own slot
        if (b1 - b0 > p.row_stride) return;
        b1 = (int64_t)i * p.row_stride + (b1 - b0);
        b0 = (int64_t)i * p.row_stride;
    }
    if (b1 > p.bytes_capacity) return;   // a row that would cross the end of the buffer is not written
    const uint32_t* row = p.counts + (int64_t)i * p.capacity;
    int64_t at = b0;
    for (int base = 0; base < nr; base += mrcnn::kWave) {
        const int j = base + lane;
        const long long x = j < nr ? string_value(row, j) : 0;
        const int k = j < nr ? rle_put_value<false>(nullptr, x) : 0;
        const int incl = wave_inclusive_scan(k, lane);
        if (j < nr) rle_put_value<true>(p.bytes + at + (incl - k), x);   // ends at most at b1 <= bytes_capacity
        at += __shfl(incl, mrcnn::kWave - 1);
    }
}

// ------------------------------------------------------------------------------------------------ rleDecode
struct DecodeParams {
    const int32_t* num_runs;
    const uint32_t* counts;
    int32_t n, capacity, h, w;
    uint8_t* out;
    int64_t image_stride, row_stride;
    uint32_t* ends;   // [n][capacity] workspace: position after run j, clipped at h*w
    int groups, nseg;
};

__global__ __launch_bounds__(kBlock) void rle_decode_ends_kernel(const DecodeParams p) {
    const int lane = threadIdx.x & (mrcnn::kWave - 1);
    const int i = blockIdx.x * kWaves + threadIdx.x / mrcnn::kWave;
    if (i >= p.n) return;
    const int nr = p.num_runs[i];
    if (!row_ok(nr, p.capacity)) return;
    const unsigned long long area = (unsigned long long)((long long)p.h * p.w);
    const int64_t row = (int64_t)i * p.capacity;
    unsigned long long end = 0;   // never above area: no sum of 64 counts overflows
    for (int base = 0; base < nr; base += mrcnn::kWave) {
        const int j = base + lane;
        unsigned long long e = end + wave_inclusive_scan((unsigned long long)(j < nr ? p.counts[row + j] : 0u), lane);
        if (e > area) e = area;
        if (j < nr) p.ends[row + j] = (uint32_t)e;
        end = __shfl(e, mrcnn::kWave - 1);
    }
}

__global__ __launch_bounds__(kBlock) void rle_decode_kernel(const DecodeParams p) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= p.groups * p.nseg) return;
    const int i = blockIdx.y;
    const int seg = t / p.groups;
    const int x0 = (t - seg * p.groups) * kCols;
    const int ncols = min(kCols, p.w - x0);
    const int y0 = seg * kSegRows, y1 = min(p.h, y0 + kSegRows);
    int nr = p.num_runs[i];
    if (!row_ok(nr, p.capacity)) nr = 0;   // a refused row decodes to zeros
    const uint32_t* ends = p.ends + (int64_t)i * p.capacity;
    int r[kCols];
    uint32_t next[kCols];
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
        r[c] = nr;
        next[c] = 0xffffffffu;
        if (c < ncols) {
            const uint32_t pos = (uint32_t)((x0 + c) * p.h + y0);   // < 2^28
            int lo = 0, hi = nr;   // ends <= pos: the run the pixel lies in
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ends[mid] <= pos) lo = mid + 1; else hi = mid;
            }
            r[c] = lo;
            if (lo < nr) next[c] = ends[lo];
        }
    }
    uint8_t* q = p.out + (int64_t)i * p.image_stride + (int64_t)y0 * p.row_stride + x0;
    for (int y = y0; y < y1; ++y) {
        uint32_t v = 0;
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            if (c < ncols) {
                const uint32_t pos = (uint32_t)((x0 + c) * p.h + y);
                while (pos >= next[c]) {   // ends are non-decreasing; an empty run is stepped over
                    ++r[c];
                    next[c] = r[c] < nr ? ends[r[c]] : 0xffffffffu;
                }
                v |= (uint32_t)(r[c] < nr ? (r[c] & 1) : 0) << (8 * c);
            }
        }
        if (ncols == kCols) {
            __builtin_memcpy(q, &v, 4);   // one dword store (global memory takes any alignment: a strided view needs no copy)
        } else {
            for (int c = 0; c < ncols; ++c) q[c] = (uint8_t)((v >> (8 * c)) & 1u);
        }
        q += p.row_stride;
    }
}

bool table_ok(int n, int capacity) { return n >= 0 && n <= kMaxRows && capacity >= 1; }
unsigned waves_grid(int n) { return (unsigned)((n + kWaves - 1) / kWaves); }

}  // namespace

extern "C" int mrcnn_rle_from_string(const uint8_t* bytes, int64_t total_bytes, const int64_t* str_off, const int32_t* heights,
                                     const int32_t* widths, int32_t n, int32_t capacity, int32_t* num_runs, uint32_t* counts,
                                     int32_t* status, mrcnn_stream_t stream) {
    MRCNN_REQUIRE(table_ok(n, capacity), "rle_from_string: n=%d must be in [0, %d], capacity=%d >= 1", n, kMaxRows, capacity);
    MRCNN_REQUIRE(total_bytes >= 0, "rle_from_string: total_bytes=%lld must be >= 0", (long long)total_bytes);
    if (n == 0) return MRCNN_OK;
    MRCNN_REQUIRE(str_off && heights && widths && num_runs && counts && status && (bytes || total_bytes == 0),
                  "rle_from_string: null pointer");
    FromStringParams p;
    p.bytes = bytes; p.str_off = str_off; p.total = total_bytes; p.heights = heights; p.widths = widths;
    p.n = n; p.capacity = capacity; p.num_runs = num_runs; p.counts = counts; p.status = status;
    hipLaunchKernelGGL(rle_from_string_kernel, dim3(waves_grid(n)), dim3(kBlock), 0, mrcnn::as_stream(stream), p);
    return mrcnn::check_launch("rle_from_string");
}

extern "C" int mrcnn_rle_area_bbox(const int32_t* num_runs, const uint32_t* counts, int32_t n, int32_t capacity,
                                   const int32_t* heights, const int32_t* widths, int32_t* areas, int32_t* bboxes,
                                   mrcnn_stream_t stream) {
    MRCNN_REQUIRE(table_ok(n, capacity), "rle_area_bbox: n=%d must be in [0, %d], capacity=%d >= 1", n, kMaxRows, capacity);
    if (n == 0) return MRCNN_OK;
    MRCNN_REQUIRE(num_runs && counts && heights && widths && areas && bboxes, "rle_area_bbox: null pointer");
    AreaParams p;
    p.num_runs = num_runs; p.counts = counts; p.heights = heights; p.widths = widths; p.n = n; p.capacity = capacity;
    p.areas = areas; p.bboxes = bboxes;
    hipLaunchKernelGGL(rle_area_bbox_kernel, dim3(waves_grid(n)), dim3(kBlock), 0, mrcnn::as_stream(stream), p);
    return mrcnn::check_launch("rle_area_bbox");
}

extern "C" size_t mrcnn_rle_to_string_workspace_bytes(int32_t n) {
    if (n <= 0 || n > kMaxRows) return 0;
    return aligned((size_t)n * sizeof(int64_t));
}

extern "C" int mrcnn_rle_to_string(const int32_t* num_runs, const uint32_t* counts, int32_t n, int32_t capacity, uint8_t* bytes,
                                   int64_t bytes_capacity, int64_t row_stride, int32_t have_offsets, int64_t* str_off,
                                   void* workspace, size_t workspace_bytes, mrcnn_stream_t stream) {
    MRCNN_REQUIRE(table_ok(n, capacity), "rle_to_string: n=%d must be in [0, %d], capacity=%d >= 1", n, kMaxRows, capacity);
    MRCNN_REQUIRE(row_stride >= 0 && (have_offsets == 0 || have_offsets == 1), "rle_to_string: row_stride=%lld (>= 0), have_offsets=%d (0 or 1)",
                  (long long)row_stride, have_offsets);
    MRCNN_REQUIRE(bytes_capacity >= 0 && str_off && (bytes || bytes_capacity == 0),
                  "rle_to_string: str_off, and bytes for a bytes_capacity=%lld above 0, must be given", (long long)bytes_capacity);
    ToStringParams p;
    p.num_runs = num_runs; p.counts = counts; p.n = n; p.capacity = capacity; p.bytes = bytes; p.bytes_capacity = bytes_capacity;
    p.str_off = str_off; p.row_bytes = static_cast<int64_t*>(workspace); p.row_stride = row_stride;
    hipStream_t s = mrcnn::as_stream(stream);
    if (n > 0) {
        MRCNN_REQUIRE(num_runs && counts, "rle_to_string: null pointer");
        const size_t need = mrcnn_rle_to_string_workspace_bytes(n);
        MRCNN_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                      "rle_to_string: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, workspace_bytes);
        if (!have_offsets) hipLaunchKernelGGL(rle_string_bytes_kernel, dim3(waves_grid(n)), dim3(kBlock), 0, s, p);
    }
    if (!have_offsets) hipLaunchKernelGGL(rle_string_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, p);   // n == 0: str_off[0] = 0
    if (n > 0 && bytes_capacity > 0) hipLaunchKernelGGL(rle_string_write_kernel, dim3(waves_grid(n)), dim3(kBlock), 0, s, p);
    return mrcnn::check_launch("rle_to_string");
}

extern "C" size_t mrcnn_rle_decode_workspace_bytes(int32_t n, int32_t capacity) {
    if (n <= 0 || capacity <= 0) return 0;
    return aligned((size_t)n * (size_t)capacity * sizeof(uint32_t));
}

extern "C" int mrcnn_rle_decode_u8(const int32_t* num_runs, const uint32_t* counts, int32_t n, int32_t capacity, int32_t height,
                                   int32_t width, uint8_t* out, int64_t image_stride, int64_t row_stride, void* workspace,
                                   size_t workspace_bytes, mrcnn_stream_t stream) {
    MRCNN_REQUIRE(n >= 0 && n <= 65535 && capacity >= 1, "rle_decode: n=%d must be in [0, 65535], capacity=%d >= 1", n, capacity);
    MRCNN_REQUIRE(height >= 1 && height <= kMaxDim && width >= 1 && width <= kMaxDim, "rle_decode: mask %dx%d (1..%d each)", height,
                  width, kMaxDim);
    MRCNN_REQUIRE(row_stride >= width, "rle_decode: row stride %lld is shorter than a row of %d pixels", (long long)row_stride,
                  width);
    MRCNN_REQUIRE(image_stride >= 0, "rle_decode: image stride %lld must be >= 0", (long long)image_stride);
    if (n == 0) return MRCNN_OK;
    MRCNN_REQUIRE(num_runs && counts && out, "rle_decode: null pointer");
    const size_t need = mrcnn_rle_decode_workspace_bytes(n, capacity);
    MRCNN_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                  "rle_decode: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, workspace_bytes);
    DecodeParams p;
    p.num_runs = num_runs; p.counts = counts; p.n = n; p.capacity = capacity; p.h = height; p.w = width;
    p.out = out; p.image_stride = image_stride; p.row_stride = row_stride;
    p.ends = static_cast<uint32_t*>(workspace);
    p.groups = (width + kCols - 1) / kCols;
    p.nseg = (height + kSegRows - 1) / kSegRows;
    hipStream_t s = mrcnn::as_stream(stream);
    hipLaunchKernelGGL(rle_decode_ends_kernel, dim3(waves_grid(n)), dim3(kBlock), 0, s, p);
    hipLaunchKernelGGL(rle_decode_kernel, dim3((unsigned)((p.groups * p.nseg + kBlock - 1) / kBlock), (unsigned)n), dim3(kBlock), 0,
                       s, p);
    return mrcnn::check_launch("rle_decode");
}
