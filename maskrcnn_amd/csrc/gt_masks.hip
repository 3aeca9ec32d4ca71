// Ground-truth masks for training, straight from run-length rows (gfx950): what CocoMaskRCNNDataset.load + encode_masks of the
// reference (data.py:797-876, :246-262) do per annotation on the host — annToMask, np.fliplr, a Pillow BILINEAR resize, a zero
// pad — for n rows of a run-list table with PER-ROW source sizes, in two launches whatever n is and however many sizes occur.
// No allocation, no host synchronisation, no atomics, the same bits from run to run; the bits are Pillow's (resample_math.hpp).
//
//   rle_resample_ends_kernel   a wave per row: the row's status bits, and (a usable row) the scan of its counts to end positions
//                              clipped at h*w — the one thing in global memory besides the output, as in rle_decode_ends_kernel
//   rle_resample_tile_kernel   a workgroup per (row, TILE_H x TILE_W tile of the CANVAS). The tile is built in LDS, zero to begin
//                              with, and stored once with 16-byte stores where base and strides allow — so the padding, a refused
//                              row and a tile the mask misses cost one store stream and nothing else. The part of the tile inside
//                              the row's placement is made in sub-tiles sized from the row's resize factor so that the SOURCE
//                              rectangle a sub-tile's taps reach (from the two axes' xmin / cnt: the bounds are monotone) fits:
//                                fill    the rectangle's on / off bytes from the run ends: runs are column-major, so one search
//                                        per (column, 16-row segment) and then a walk; the mirror is x -> w-1-x here
//                                h pass  LDS -> LDS, the 8-bit intermediate with its rounding ([rows_in][sub-tile columns])
//                                v pass  LDS -> the tile
//                              A sub-tile whose rectangle holds no on pixel is skipped: the resample of zeros is zero.
//   An axis whose new size equals its source size is not resampled (Pillow skips that pass): one tap of weight 2^22, which is
//   the identity on bytes. No dense source mask and no horizontal-pass intermediate ever reach global memory.
#include "common.hpp"
#include "resample_math.hpp"
#include "workgroup.hpp"

namespace {

using namespace mrcnn_resample;
using mrcnn::wave_inclusive_scan;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / mrcnn::kWave;
constexpr int kMaxDim = 16384;
constexpr int kMaxShrink = 16;                  // source size <= kMaxShrink * new size, per axis
constexpr int KMAX = 2 * kMaxShrink + 1;        // taps of one output sample at that factor
constexpr int TILE_H = 32, TILE_W = 64;         // canvas pixels per workgroup
constexpr int ROWS_MAX = 66, COLS_MAX = 104;    // source rectangle of one sub-tile: 36 x 68 for a whole tile when enlarging, 54 x 102
constexpr int SRC_STRIDE = 104;                 // at a factor of 1.5, 66 x 98 for 2 x 4 outputs at the limit of 16; 26 KB of LDS in all
constexpr int kFillRows = 16;                   // source rows per search
constexpr size_t kAlign = 256;
size_t aligned(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

enum : int32_t { kUnusableRow = 1, kBadSize = 2, kBadPlacement = 4, kShrinkLimit = 8 };

struct ResampleParams {
    const int32_t* num_runs;
    const uint32_t* counts;
    const int32_t* heights;
    const int32_t* widths;
    const int32_t* geom;   // [n][5]: new_h, new_w, top, left, flip
    int32_t n, capacity, out_h, out_w;
    uint8_t* out;
    int64_t image_stride, row_stride;
    int32_t* status;
    uint32_t* ends;        // [n][capacity] workspace: position after run j, clipped at h*w
    int tiles_x;
    int vec;               // base and strides are multiples of 16: a tile row is stored in 16-byte groups
};

__device__ __forceinline__ bool dim_ok(int v) { return v >= 1 && v <= kMaxDim; }

__global__ __launch_bounds__(kBlock) void rle_resample_ends_kernel(const ResampleParams p) {
    const int lane = threadIdx.x & (mrcnn::kWave - 1);
    const int i = blockIdx.x * kWaves + threadIdx.x / mrcnn::kWave;   // wave-uniform
    if (i >= p.n) return;
    const int nr = p.num_runs[i];
    const int h = p.heights[i], w = p.widths[i];
    const int32_t* g = p.geom + 5 * (int64_t)i;
    const int new_h = g[0], new_w = g[1], top = g[2], left = g[3];
    int32_t st = 0;
    if (nr < 0 || nr > p.capacity) st |= kUnusableRow;
    const bool sizes = dim_ok(h) && dim_ok(w) && dim_ok(new_h) && dim_ok(new_w);
    if (!sizes) st |= kBadSize;
    if (top < 0 || left < 0 || (int64_t)top + new_h > p.out_h || (int64_t)left + new_w > p.out_w) st |= kBadPlacement;
    if (sizes && (h > kMaxShrink * new_h || w > kMaxShrink * new_w)) st |= kShrinkLimit;
    if (lane == 0) p.status[i] = st;
    if (st) return;
    const unsigned long long area = (unsigned long long)((long long)h * w);
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

// the coefficients of output sample xx of one axis: Pillow's, or the single unit tap of an axis that is not resampled
__device__ __forceinline__ void sample_coeffs(const Axis& a, int xx, int& xmin, int& cnt, int* k) {
    if (a.in_size == a.out_size) {
        xmin = xx;
        cnt = 1;
        k[0] = 1 << PRECISION_BITS;
        return;
    }
    axis_coeffs(a, xx, xmin, cnt, k, 1);
}

// Output samples per sub-tile along one axis, at most `full`: the source samples s outputs reach are at most
// (s-1)*scale + 2*support + 2 (both ends are truncations of center -+ support + 0.5), which must stay within `limit`.
__device__ __forceinline__ int sub_tile(const Axis& a, int full, int limit) {
    if (a.in_size == a.out_size) return full;   // full <= limit
    int s = full;
    while (s > 1 && static_cast<int>(ceil(s * a.scale)) + 2 * static_cast<int>(ceil(a.support)) + 2 > limit) s >>= 1;
    return s;
}

// The first j in [0, nr] with ends[j] > pos (nr: none), ends non-decreasing: a search with SEVEN probes a step. The probes of a
// step are independent loads, so a row of 500 runs costs three memory latencies where the binary search pays nine — and the
// fill, a chain of dependent loads from L2 in front of everything else a workgroup does, is what the kernel's time is made of.
__device__ __forceinline__ int first_end_above(const uint32_t* __restrict__ ends, int nr, uint32_t pos) {
    int lo = 0, hi = nr;   // the answer lies in [lo, hi]
    while (hi - lo > 8) {
        const int step = (hi - lo) >> 3;   // >= 1; probe j at lo + j*step < hi
        int c = 0;
#pragma unroll
        for (int j = 1; j <= 7; ++j) c += ends[lo + j * step] <= pos ? 1 : 0;   // a prefix of the probes: ends are sorted
        const int base = lo;
        if (c < 7) hi = base + (c + 1) * step;   // ends[hi] > pos
        if (c > 0) lo = base + c * step + 1;     // ends[lo - 1] <= pos
    }
    int c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) c += (lo + j < hi && ends[lo + j] <= pos) ? 1 : 0;
    return lo + c;
}

__global__ __launch_bounds__(kBlock) void rle_resample_tile_kernel(const ResampleParams p) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) unsigned char out_lds[TILE_H * TILE_W];
    __shared__ __attribute__((aligned(16))) unsigned char src_lds[ROWS_MAX * SRC_STRIDE];
    __shared__ __attribute__((aligned(16))) unsigned char mid_lds[ROWS_MAX * TILE_W];
    __shared__ int kh[TILE_W * KMAX], kv[TILE_H * KMAX], bh[2 * TILE_W], bv[2 * TILE_H];
    const int tid = threadIdx.x;
    const int k = blockIdx.y;
    const int tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;
    const int X0 = tx * TILE_W, Y0 = ty * TILE_H;
    for (int i = tid; i < TILE_H * TILE_W / 4; i += kBlock) reinterpret_cast<unsigned*>(out_lds)[i] = 0u;

    // everything below up to the store is workgroup-uniform control flow
    int lx0 = 0, lx1 = 0, ly0 = 0, ly1 = 0, h = 1, w = 1, new_h = 1, new_w = 1, top = 0, left = 0, flip = 0;
    if (p.status[k] == 0) {   // a refused row is all zeros
        const int32_t* g = p.geom + 5 * (int64_t)k;
        h = p.heights[k]; w = p.widths[k];
        new_h = g[0]; new_w = g[1]; top = g[2]; left = g[3]; flip = g[4] != 0;
        lx0 = max(left - X0, 0); lx1 = min(left + new_w - X0, TILE_W);     // the placement within this tile
        ly0 = max(top - Y0, 0);  ly1 = min(top + new_h - Y0, TILE_H);
    }
    const Axis ah = make_axis(w, new_w), av = make_axis(h, new_h);
    const int ksh = w == new_w ? 1 : ah.ksize, ksv = h == new_h ? 1 : av.ksize;
    if (lx0 < lx1 && ly0 < ly1 && ksh <= KMAX && ksv <= KMAX) {
        if (tid < TILE_W) {
            if (tid >= lx0 && tid < lx1) {
                int xmin, cnt;
                sample_coeffs(ah, X0 + tid - left, xmin, cnt, kh + tid * ksh);
                bh[2 * tid] = xmin;
                bh[2 * tid + 1] = cnt;
            }
        } else if (tid < TILE_W + TILE_H) {
            const int j = tid - TILE_W;
            if (j >= ly0 && j < ly1) {
                int ymin, cnt;
                sample_coeffs(av, Y0 + j - top, ymin, cnt, kv + j * ksv);
                bv[2 * j] = ymin;
                bv[2 * j + 1] = cnt;
            }
        }
        __syncthreads();
        const int nr = p.num_runs[k];
        const uint32_t* ends = p.ends + (int64_t)k * p.capacity;
        const int sw = sub_tile(ah, TILE_W, COLS_MAX), sh = sub_tile(av, TILE_H, ROWS_MAX);
        for (int sy = ly0; sy < ly1; sy += sh) {
            for (int sx = lx0; sx < lx1; sx += sw) {
                const int ey = min(sy + sh, ly1), ex = min(sx + sw, lx1);
                // the source rows and columns the sub-tile reads
                const int in0 = bv[2 * sy], rows_in = bv[2 * (ey - 1)] + bv[2 * (ey - 1) + 1] - in0;
                const int c0 = bh[2 * sx], cols_in = bh[2 * (ex - 1)] + bh[2 * (ex - 1) + 1] - c0;
                // never taken (sub_tile's bound); the buffers are not to be overrun whatever the coefficients say
                if (rows_in < 1 || cols_in < 1 || rows_in > ROWS_MAX || cols_in > COLS_MAX || in0 < 0 || c0 < 0 ||
                    in0 + rows_in > h || c0 + cols_in > w)
                    continue;
                // ---- fill: a thread owns kFillRows rows of one source column
                const int chunks = (rows_in + kFillRows - 1) / kFillRows;
                unsigned any = 0;
                for (int it = tid; it < cols_in * chunks; it += kBlock) {
                    const int ch = it / cols_in, c = it - ch * cols_in;
                    const int r0 = ch * kFillRows, r1 = min(r0 + kFillRows, rows_in);
                    const int x = flip ? w - 1 - (c0 + c) : c0 + c;
                    uint32_t pos = (uint32_t)(x * h + in0 + r0);   // < 2^28
                    int lo = first_end_above(ends, nr, pos);       // the run the pixel lies in
                    uint32_t next = lo < nr ? ends[lo] : 0xffffffffu;
                    for (int r = r0; r < r1; ++r, ++pos) {
                        while (pos >= next) {   // ends are non-decreasing; an empty run is stepped over
                            ++lo;
                            next = lo < nr ? ends[lo] : 0xffffffffu;
                        }
                        const unsigned v = lo < nr ? (unsigned)(lo & 1) : 0u;
                        src_lds[r * SRC_STRIDE + c] = (unsigned char)v;
                        any |= v;
                    }
                }
                if (!__syncthreads_or((int)any)) continue;   // zeros in, zeros out: the tile is zero already
                // ---- horizontal pass into the 8-bit intermediate
                const int cw = ex - sx;
                for (int it = tid; it < rows_in * cw; it += kBlock) {
                    const int r = it / cw, j = it - r * cw, J = sx + j;
                    const int cnt = bh[2 * J + 1];
                    const int* kk = kh + J * ksh;
                    const unsigned char* s = src_lds + r * SRC_STRIDE + (bh[2 * J] - c0);
                    int ss = 1 << (PRECISION_BITS - 1);
                    for (int t = 0; t < cnt; ++t) ss += s[t] * kk[t];
                    mid_lds[r * TILE_W + j] = (unsigned char)clip8(ss);
                }
                __syncthreads();
                // ---- vertical pass into the tile
                for (int it = tid; it < (ey - sy) * cw; it += kBlock) {
                    const int i = it / cw, j = it - i * cw, I = sy + i;
                    const int cnt = bv[2 * I + 1];
                    const int* kk = kv + I * ksv;
                    const unsigned char* s = mid_lds + (bv[2 * I] - in0) * TILE_W + j;
                    int ss = 1 << (PRECISION_BITS - 1);
                    for (int t = 0; t < cnt; ++t) ss += s[t * TILE_W] * kk[t];
                    out_lds[I * TILE_W + sx + j] = (unsigned char)clip8(ss);
                }
                // the next sub-tile's fill touches src_lds only, and its barrier stands before mid_lds is written again
            }
        }
    }
    __syncthreads();
    // ---- store the part of the tile that lies on the out_h x out_w extent: a thread owns sixteen bytes of a tile row
    uint8_t* obase = p.out + (int64_t)k * p.image_stride;
    for (int gi = tid; gi < TILE_H * (TILE_W / 16); gi += kBlock) {
        const int ry = gi / (TILE_W / 16), gx = (gi - ry * (TILE_W / 16)) * 16;
        const int Y = Y0 + ry, X = X0 + gx;
        if (Y >= p.out_h || X >= p.out_w) continue;
        uint8_t* q = obase + (int64_t)Y * p.row_stride + X;
        const unsigned char* s = out_lds + ry * TILE_W + gx;
        if (p.vec && X + 16 <= p.out_w) {
            *reinterpret_cast<u32x4*>(q) = *reinterpret_cast<const u32x4*>(s);
        } else {
            const int m = min(16, p.out_w - X);
            for (int j = 0; j < m; ++j) q[j] = s[j];
        }
    }
}

}  // namespace

extern "C" size_t mrcnn_rle_resample_workspace_bytes(int32_t n, int32_t capacity) {
    if (n <= 0 || capacity <= 0) return 0;
    return aligned((size_t)n * (size_t)capacity * sizeof(uint32_t));
}

extern "C" int mrcnn_rle_resample_u8(const int32_t* num_runs, const uint32_t* counts, int32_t n, int32_t capacity,
                                     const int32_t* heights, const int32_t* widths, const int32_t* geom, uint8_t* out,
                                     int32_t out_h, int32_t out_w, int64_t image_stride, int64_t row_stride, int32_t* status,
                                     void* workspace, size_t workspace_bytes, mrcnn_stream_t stream) {
    MRCNN_REQUIRE(n >= 0 && n <= 65535 && capacity >= 1, "rle_resample: n=%d must be in [0, 65535], capacity=%d >= 1", n, capacity);
    MRCNN_REQUIRE(out_h >= 1 && out_h <= kMaxDim && out_w >= 1 && out_w <= kMaxDim, "rle_resample: canvas %dx%d (1..%d each)", out_h,
                  out_w, kMaxDim);
    MRCNN_REQUIRE(row_stride >= out_w, "rle_resample: row stride %lld is shorter than a row of %d pixels", (long long)row_stride,
                  out_w);
    MRCNN_REQUIRE(image_stride >= 0, "rle_resample: image stride %lld must be >= 0", (long long)image_stride);
    if (n == 0) return MRCNN_OK;
    MRCNN_REQUIRE(num_runs && counts && heights && widths && geom && out && status, "rle_resample: null pointer");
    const size_t need = mrcnn_rle_resample_workspace_bytes(n, capacity);
    MRCNN_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                  "rle_resample: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, workspace_bytes);
    ResampleParams p;
    p.num_runs = num_runs; p.counts = counts; p.heights = heights; p.widths = widths; p.geom = geom;
    p.n = n; p.capacity = capacity; p.out_h = out_h; p.out_w = out_w;
    p.out = out; p.image_stride = image_stride; p.row_stride = row_stride;
    p.status = status; p.ends = static_cast<uint32_t*>(workspace);
    p.tiles_x = (out_w + TILE_W - 1) / TILE_W;
    p.vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0 && image_stride % 16 == 0 && row_stride % 16 == 0;
    const int tiles_y = (out_h + TILE_H - 1) / TILE_H;
    hipStream_t s = mrcnn::as_stream(stream);
    hipLaunchKernelGGL(rle_resample_ends_kernel, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(kBlock), 0, s, p);
    hipLaunchKernelGGL(rle_resample_tile_kernel, dim3((unsigned)(p.tiles_x * tiles_y), (unsigned)n), dim3(kBlock), 0, s, p);
    return mrcnn::check_launch("rle_resample");
}
