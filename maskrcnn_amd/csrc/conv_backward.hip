// Backward of the fp32 NHWC convolution with a frozen affine and an activation (the layers train_model trains, model.py:1010-1016;
// stride 1 for the heads, stride 2 for the stem and the first block of C3 / C4 / C5): gradients for the input, the weight, the
// shift and the residual. The rule is stated at mrcnn_conv_act_backward_f32 in include/maskrcnn_hip.h, for both strides. Built
// with -ffp-contract=off: g and z are separately rounded operations.
//   conv_act_backward   elementwise: dy, y -> z (= g * scale, pitch Cout4), g, the 2 x 2 residual sums, and per (workgroup, thread
//                       row) fp64 partials of dshift — a thread owns channel quads and walks its pixels in ascending order.
//   conv_weight_flip    w [Cout][KH][KW][Cin] -> w' [Cin][KH][KW][Cout4], taps mirrored: the data gradient is then the FORWARD
//                       (mrcnn_conv_bn_act_nhwc_f32) on z, bit for bit, with its routes and limits.
//   conv_wgrad_f32      the weight gradient as a GEMM with M' = Cout, N' = KH*KW*Cin, K' = the pixels of one chunk. Both operands
//                       lie "k-major with the other index contiguous" already (a z row is a run of co, an x row at a tap a run
//                       of ci), so a k tile of 32 pixels goes to LDS as it lies and a lane fetches its one-register A / B
//                       operand of v_mfma_f32_32x32x2_f32 with a ds_read_b32 along the channel run (32 consecutive floats per
//                       lane group: conflict-free at any pitch). MFMA step s of a k tile contracts pixels 2s (lanes 0-31) and
//                       2s + 1 (lanes 32-63): an element is an fmaf chain over the chunk's pixels in ascending order.
//   conv_wgrad_reduce   the chunks' sums (or dshift's partials) in index order in fp64, narrowed last.
// No floating-point atomic, no last-block protocol, no inline assembly; nothing here synchronises with the host.
#include "conv_common.hpp"

namespace {

using namespace mrcnn_conv;

constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------------ g, z, residual sums, dshift
struct ActBackwardParams {
    const float* dy;
    const float* y;
    const float* scale;
    const int* row_counts;
    float* z;
    float* g;
    float* dres2;
    double* part;   // [workgroups * RT][C4]
    int M, OH, OW, C, C4, act, scatter, rows_per_group;
    int units, units_per_block, CT, RT;   // a unit: one GEMM row, or one 2 x 2 block of them (RES2)
};

// Element offset of GEMM element (row m, column n) in dy / y: dense, or the 2 x 2 scatter of the transposed conv.
__device__ __forceinline__ int act_elem(const ActBackwardParams& p, int m, int n) {
    if (!p.scatter) return m * p.C + n;
    const int cq = p.C >> 2, ohw = p.OH * p.OW;
    const int b = m / ohw, rem = m - b * ohw, i = rem / p.OW, j = rem - i * p.OW;
    const int q = n / cq, co = n - q * cq;
    return ((b * 2 * p.OH + 2 * i + (q >> 1)) * (2 * p.OW) + 2 * j + (q & 1)) * cq + co;
}

template <bool RES2>
__global__ __launch_bounds__(kThreads) void conv_act_backward(const ActBackwardParams p) {
    constexpr int NPX = RES2 ? 4 : 1;
    const int tx = threadIdx.x % p.CT, ty = threadIdx.x / p.CT;
    const int u0 = blockIdx.x * p.units_per_block, u1 = min(u0 + p.units_per_block, p.units);
    const int quads = p.C4 >> 2;
    // 16-byte accesses where a quad of columns is a run of four floats on a 16-byte boundary in dy / y
    const bool vec = (p.C & 3) == 0 && (!p.scatter || ((p.C >> 2) & 3) == 0);
    for (int cq = tx; cq < quads; cq += p.CT) {
        const int c0 = cq * 4;
        float sc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) sc[k] = (p.scale && c0 + k < p.C) ? p.scale[c0 + k] : 1.0f;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int u = u0 + ty; u < u1; u += p.RT) {
            float gs[NPX][4];
#pragma unroll
            for (int q = 0; q < NPX; ++q) {
                int m = u;
                if constexpr (RES2) {
                    const int hw2 = (p.OH >> 1) * (p.OW >> 1), w2 = p.OW >> 1;
                    const int b = u / hw2, rem = u - b * hw2, i = rem / w2, j = rem - i * w2;
                    m = (b * p.OH + 2 * i + (q >> 1)) * p.OW + 2 * j + (q & 1);
                }
                bool valid = true;
                if (p.row_counts) {
                    const int grp = m / p.rows_per_group;
                    valid = m - grp * p.rows_per_group < p.row_counts[grp];
                }
                float d[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
                if (valid) {   // an invalid row's dy and y are never read
                    if (vec) {
                        const int e = act_elem(p, m, c0);
                        const float4 t = *reinterpret_cast<const float4*>(p.dy + e);
                        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
                        if (p.act) {
                            const float4 s = *reinterpret_cast<const float4*>(p.y + e);
                            v[0] = s.x; v[1] = s.y; v[2] = s.z; v[3] = s.w;
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (c0 + k < p.C) {
                                const int e = act_elem(p, m, c0 + k);
                                d[k] = p.dy[e];
                                if (p.act) v[k] = p.y[e];
                            }
                    }
                }
                float zq[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float gk = d[k];
                    if (p.act == 1) gk = v[k] > 0.f ? d[k] : 0.f;
                    if (p.act == 2) {
                        const float t = 1.0f - v[k];
                        const float uu = v[k] * t;
                        gk = d[k] * uu;
                    }
                    if (!valid || c0 + k >= p.C) gk = 0.f;
                    gs[q][k] = gk;
                    zq[k] = p.scale ? gk * sc[k] : gk;
                    if (valid) acc[k] += static_cast<double>(gk);
                }
                if (p.z) *reinterpret_cast<float4*>(p.z + static_cast<size_t>(m) * p.C4 + c0) = make_float4(zq[0], zq[1], zq[2], zq[3]);
                if (p.g) {
                    float* gp = p.g + static_cast<size_t>(m) * p.C + c0;
                    if ((p.C & 3) == 0) *reinterpret_cast<float4*>(gp) = make_float4(gs[q][0], gs[q][1], gs[q][2], gs[q][3]);
                    else
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (c0 + k < p.C) gp[k] = gs[q][k];
                }
            }
            if constexpr (RES2) {
                float* rp = p.dres2 + static_cast<size_t>(u) * p.C + c0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c0 + k < p.C) rp[k] = (gs[0][k] + gs[1][k]) + (gs[2][k] + gs[3][k]);
            }
        }
        if (p.part) {
            double* pp = p.part + (static_cast<size_t>(blockIdx.x) * p.RT + ty) * p.C4 + c0;
#pragma unroll
            for (int k = 0; k < 4; ++k) pp[k] = acc[k];
        }
    }
}

// The geometry of conv_act_backward: a function of the shape only (it fixes dshift's summation order).
struct ActGeometry {
    int CT, RT, units, units_per_block, blocks;
};
inline ActGeometry act_geometry(long long M, int C4, bool res2) {
    ActGeometry a;
    const int quads = C4 / 4;
    a.CT = 1;
    while (a.CT < quads && a.CT < 64) a.CT *= 2;
    a.RT = kThreads / a.CT;
    a.units = static_cast<int>(res2 ? M / 4 : M);
    long long blocks = (a.units + 8LL * a.RT - 1) / (8LL * a.RT);   // eight units per thread, at most 256 workgroups
    blocks = std::max(1LL, std::min(blocks, 256LL));
    a.units_per_block = static_cast<int>((a.units + blocks - 1) / blocks);
    a.blocks = (a.units + a.units_per_block - 1) / a.units_per_block;
    return a;
}
inline size_t act_partial_bytes(long long M, int C4) {
    const ActGeometry a = act_geometry(M, C4, false);   // the 2 x 2 form has a quarter of the units: never more partials
    return sizeof(double) * static_cast<size_t>(a.blocks) * a.RT * C4;
}

// ------------------------------------------------------------------------------------------------ partial sums -> result
// out[e] = fp32( sum over i < n, ascending, of fp64(part[i * stride + e]) ), e < count.
template <typename T>
__global__ __launch_bounds__(kThreads) void conv_wgrad_reduce(const T* __restrict__ part, long long stride, int n, long long count,
                                                              float* __restrict__ out) {
    const long long e = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x;
    if (e >= count) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += static_cast<double>(part[i * stride + e]);
    out[e] = static_cast<float>(s);
}

template <typename T>
int launch_reduce(const T* part, long long stride, int n, long long count, float* out, hipStream_t s) {
    const long long blocks = (count + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(conv_wgrad_reduce<T>, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, part, stride, n, count, out);
    return mrcnn::check_launch("conv_wgrad_reduce");
}

// ------------------------------------------------------------------------------------------------ w -> w'
__global__ __launch_bounds__(kThreads) void conv_weight_flip(const float* __restrict__ w, int cout, int cout4, int kh, int kw, int cin,
                                                             float* __restrict__ wt) {
    const long long total = 1LL * cin * kh * kw * cout4;
    const long long e = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x;
    if (e >= total) return;
    const int co = static_cast<int>(e % cout4);
    long long r = e / cout4;
    const int kx = static_cast<int>(r % kw);
    r /= kw;
    const int ky = static_cast<int>(r % kh), ci = static_cast<int>(r / kh);
    wt[e] = co < cout ? w[((1LL * co * kh + (kh - 1 - ky)) * kw + (kw - 1 - kx)) * cin + ci] : 0.f;
}

// ------------------------------------------------------------------------------------------------ the weight gradient
struct WgradParams {
    const float* x;   // [B][H][W][Cin]
    const float* z;   // [M][Cout4]
    float* part;      // [chunks][Cout][N]
    const int* row_counts;
    int rows_per_group;
    int H, W, Cin, Cout, Cout4, KW, pad_t, pad_l, OH, OW, stride;
    int M, N, L, tiles_m, tiles_n;
    unsigned x_bytes, z_bytes;
};

constexpr int WG_BN = 128, WG_BK = 32;   // columns (taps x input channels) of a workgroup tile; pixels of a k tile
template <int BM>
constexpr size_t wgrad_lds_bytes() {
    return sizeof(float) * 2 * WG_BK * (BM + WG_BN) + sizeof(int4) * 2 * WG_BK;
}
// Rows (output channels) of the workgroup tile: the narrowest that holds Cout, so that the RPN's 18-channel head or a 36-channel
// FC does not run a tile of which three quarters is padding.
inline int wgrad_bm(int cout) { return cout <= 32 ? 32 : cout <= 64 ? 64 : 128; }
// The chunk length L: the pixels are cut so that a 256-CU part gets AT MOST two workgroups per CU (512, what its LDS holds) over
// all tiles — one resident wave of workgroups: a workgroup walks hundreds of k tiles, and 576 of them (the RPN shared conv with
// the count rounded up) ran as a full round and a round of 64, 1.55 x the forward's time with the CUs busy for 1.22 x —, in whole
// k tiles and never fewer than four of them (a chunk ends with a BM x 128 store of its sums). A function of the shape only.
inline int wgrad_chunk(long long M, int cout, long long N) {
    const int bm = wgrad_bm(cout);
    const long long tiles = ((cout + bm - 1) / bm) * ((N + WG_BN - 1) / WG_BN);
    const long long want = std::max(1LL, 512 / tiles);
    long long L = (M + want - 1) / want;
    L = (L + WG_BK - 1) / WG_BK * WG_BK;
    return static_cast<int>(std::max<long long>(L, 4 * WG_BK));
}

template <int BM, int WM, int WN>
__global__ __launch_bounds__(kThreads, 2) void conv_wgrad_f32(const WgradParams p) {
    constexpr int BN = WG_BN, BK = WG_BK;
    constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);   // 32 x 32 MFMA tiles per wave
    constexpr int ZS = BM / 4;                                 // 16-byte slots per staged z row
    constexpr int PZ = BK * ZS / kThreads, PX = BK * (BN / 4) / kThreads;   // slots per thread and k tile
    static_assert(WM * WN == 4 && TM >= 1 && TN >= 1 && PZ >= 1 && PX == 4, "four waves");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Zs = smem;                      // [2][BK][BM]
    float* Xs = smem + 2 * BK * BM;        // [2][BK][BN]
    int4* tbl = reinterpret_cast<int4*>(Xs + 2 * BK * BN);   // [2][BK]: (x element offset, iy0, ix0, z byte offset) of a k tile's pixels

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ln = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int tn = blockIdx.x % p.tiles_n, rest = blockIdx.x / p.tiles_n;
    const int tm = rest % p.tiles_m, chunk = rest / p.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int mbeg = chunk * p.L, mend = min(mbeg + p.L, p.M);   // chunk * L < M: no overflow
    const int nk = (mend - mbeg + BK - 1) / BK;

    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t z_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.z), 0, p.z_bytes, 0x00020000);
    auto bload = [](const __amdgpu_buffer_rsrc_t& r, unsigned byte_off) -> float4 {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, static_cast<int>(byte_off), 0, 0);
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    };

    // The thread's x slot is one 16-byte column of the tile for the whole kernel: its tap is decoded once (Cin % 4 == 0: a slot
    // lies inside one tap; the tile may straddle taps).
    const int xc = tid & 31, xr = tid >> 5;   // column slot, first row; rows xr + 8 i
    const int ncol = n0 + 4 * xc;
    const bool col_ok = ncol < p.N;
    int ky = 0, kx = 0, tap_off = 0;
    if (col_ok) {
        const int tap = ncol / p.Cin, ci = ncol - tap * p.Cin;
        ky = tap / p.KW;
        kx = tap - ky * p.KW;
        tap_off = (ky * p.W + kx) * p.Cin + ci;
    }
    // z slots: e = tid + 256 i -> row e / ZS, column slot e % ZS
    unsigned zcol[PZ];
    int zrow[PZ];
#pragma unroll
    for (int i = 0; i < PZ; ++i) {
        const int e = tid + kThreads * i;
        zrow[i] = e / ZS;
        const int co = m0 + 4 * (e % ZS);
        zcol[i] = co < p.Cout4 ? static_cast<unsigned>(co) * 4u : OOB;
    }

    // One entry per pixel of a k tile, made by the first 32 threads: the pixel's decode costs two divisions, and 256 threads
    // repeating it for their four rows would be VALU work beside the MFMAs. A pixel past the chunk's end, past M or in an invalid
    // row gets a row nothing can match (iy0 far outside) and a z offset out of range: its x and z are never read.
    auto make_table = [&](int kt, int slot) {
        if (tid < BK) {
            const int m = mbeg + kt * BK + tid;
            bool ok = kt < nk && m < mend;
            const int mm = ok ? m : 0;
            if (ok && p.row_counts) {
                const int grp = mm / p.rows_per_group;
                ok = mm - grp * p.rows_per_group < p.row_counts[grp];
            }
            const int ohw = p.OH * p.OW;
            const int b = mm / ohw, rem = mm - b * ohw, oy = rem / p.OW, ox = rem - oy * p.OW;
            int4 e;
            e.y = ok ? oy * p.stride - p.pad_t : -(1 << 24);
            e.z = ox * p.stride - p.pad_l;
            e.x = ok ? ((b * p.H + e.y) * p.W + e.z) * p.Cin : 0;
            e.w = ok ? static_cast<int>(static_cast<unsigned>(mm) * static_cast<unsigned>(p.Cout4) * 4u) : static_cast<int>(OOB);
            tbl[slot * BK + tid] = e;
        }
    };
    float4 rz[PZ], rx[PX];
    auto issue = [&](int slot) {   // the global loads of the k tile whose table is in `slot`
#pragma unroll
        for (int i = 0; i < PZ; ++i) {
            const int4 e = tbl[slot * BK + zrow[i]];
            rz[i] = bload(z_rsrc, oob_add(static_cast<unsigned>(e.w), zcol[i]));
        }
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const int4 e = tbl[slot * BK + xr + 8 * i];
            const bool ok = col_ok && static_cast<unsigned>(e.y + ky) < static_cast<unsigned>(p.H) &&
                            static_cast<unsigned>(e.z + kx) < static_cast<unsigned>(p.W);
            rx[i] = bload(x_rsrc, ok ? static_cast<unsigned>(e.x + tap_off) * 4u : OOB);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < PZ; ++i) {
            const int e = tid + kThreads * i;
            *reinterpret_cast<float4*>(Zs + (buf * BK + zrow[i]) * BM + 4 * (e % ZS)) = rz[i];
        }
#pragma unroll
        for (int i = 0; i < PX; ++i) *reinterpret_cast<float4*>(Xs + (buf * BK + xr + 8 * i) * BN + 4 * xc) = rx[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    make_table(0, 0);
    make_table(1, 1);
    __syncthreads();
    issue(0);
    stash(0);
    __syncthreads();
    // k tile kt: its operands are in LDS buffer kt & 1, the table of k tile kt + 1 in slot (kt + 1) & 1. The loads of k tile kt + 1
    // are issued in front of the MFMAs and written to the other buffer behind them; the table of k tile kt + 2 replaces the one
    // the loads of k tile kt read before the last barrier. One barrier per k tile.
    const float* za = Zs + wm * (TM * 32) + ln;
    const float* xb = Xs + wn * (TN * 32) + ln;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        const bool more = kt + 1 < nk;   // uniform
        if (more) issue(buf ^ 1);
        make_table(kt + 2, buf);
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            const int row = buf * BK + 2 * s + lh;
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = za[row * BM + i * 32];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = xb[row * BN + j * 32];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) stash(buf ^ 1);
        __syncthreads();
    }

    // the chunk's sums: part[chunk][co][n], 128-byte runs of n per lane group; 64-bit offsets
    float* out = p.part + static_cast<size_t>(chunk) * p.Cout * p.N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * (TN * 32) + j * 32 + ln;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = m0 + wm * (TM * 32) + i * 32 + 4 * lh + (r & 3) + 8 * (r >> 2);
                if (co < p.Cout && n < p.N) out[static_cast<size_t>(co) * p.N + n] = acc[i][j][r];
            }
        }
}

// ------------------------------------------------------------------------------------------------ host
struct BackwardShape {
    int B, H, W, Cin, Cout, Cout4, KH, KW, pt, pl, pb, pr, OH, OW, stride;
    long long M, N;
};

// The limits of the data and weight gradients and the two queries, checked before any launch.
int fill_shape(BackwardShape& s, const char* who, int batch, int height, int width, int cin, int cout, int kh, int kw, int stride,
               int pad_top, int pad_left, int pad_bottom, int pad_right) {
    if (!(stride == 1 || stride == 2)) return mrcnn::fail(MRCNN_ERR_INVALID_ARGUMENT, "%s: stride must be 1 or 2, got %d", who, stride);
    if (!(batch >= 1 && height >= 1 && width >= 1 && cin >= 4 && cin % 4 == 0 && cout >= 1))
        return mrcnn::fail(MRCNN_ERR_INVALID_ARGUMENT, "%s: bad shape B=%d H=%d W=%d Cin=%d (Cin %% 4 == 0 required) Cout=%d", who,
                           batch, height, width, cin, cout);
    if (!(kh >= 1 && kw >= 1 && pad_top >= 0 && pad_left >= 0 && pad_bottom >= 0 && pad_right >= 0))
        return mrcnn::fail(MRCNN_ERR_INVALID_ARGUMENT, "%s: bad kernel/pad", who);
    if (!(pad_top <= kh - 1 && pad_bottom <= kh - 1 && pad_left <= kw - 1 && pad_right <= kw - 1))
        return mrcnn::fail(MRCNN_ERR_INVALID_ARGUMENT, "%s: a pad larger than the kernel size - 1 (the data gradient's pads are K - 1 - pad)", who);
    s.B = batch; s.H = height; s.W = width; s.Cin = cin; s.Cout = cout; s.KH = kh; s.KW = kw;
    s.pt = pad_top; s.pl = pad_left; s.pb = pad_bottom; s.pr = pad_right;
    s.stride = stride;
    if (!(height + pad_top + pad_bottom >= kh && width + pad_left + pad_right >= kw))
        return mrcnn::fail(MRCNN_ERR_INVALID_ARGUMENT, "%s: empty output", who);
    s.OH = (height + pad_top + pad_bottom - kh) / stride + 1;
    s.OW = (width + pad_left + pad_right - kw) / stride + 1;
    if (cout > 0x7ffffff0) return mrcnn::fail(MRCNN_ERR_INVALID_ARGUMENT, "%s: tensor too large", who);
    s.Cout4 = (cout + 3) / 4 * 4;
    s.M = 1LL * batch * s.OH * s.OW;
    s.N = 1LL * kh * kw * cin;
    if (!(4LL * batch * height * width * cin <= MAX_BUFFER_BYTES && 4LL * s.M * s.Cout4 <= MAX_BUFFER_BYTES &&
          4LL * s.N * s.Cout4 <= MAX_BUFFER_BYTES && s.M < (1LL << 31)))
        return mrcnn::fail(MRCNN_ERR_INVALID_ARGUMENT,
                           "%s: tensor too large (each tensor, z included, <= 0xFFFFFFF0 bytes: 32-bit buffer byte offsets)", who);
    return MRCNN_OK;
}

inline size_t wgrad_partial_bytes(const BackwardShape& s) {
    const int L = wgrad_chunk(s.M, s.Cout, s.N);
    return sizeof(float) * static_cast<size_t>((s.M + L - 1) / L) * s.Cout * s.N;
}
inline size_t backward_workspace_bytes(const BackwardShape& s) {
    return std::max({act_partial_bytes(s.M, s.Cout4), sizeof(float) * static_cast<size_t>(s.N) * s.Cout4, wgrad_partial_bytes(s)});
}

template <int BM, int WM, int WN>
int launch_wgrad(WgradParams& p, int chunks, hipStream_t stream) {
    p.tiles_m = (p.Cout + BM - 1) / BM;
    p.tiles_n = (p.N + WG_BN - 1) / WG_BN;
    const long long grid = 1LL * chunks * p.tiles_m * p.tiles_n;
    if (grid > 0x7fffffffLL) return mrcnn::fail(MRCNN_ERR_UNSUPPORTED, "conv_backward_weights: grid too large");
    return mrcnn::launch_kernel(conv_wgrad_f32<BM, WM, WN>, grid, kThreads, wgrad_lds_bytes<BM>(), stream, "conv_backward_weights",
                                "conv_wgrad_f32", p);
}

}  // namespace

extern "C" size_t mrcnn_conv_backward_workspace_bytes(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t cout,
                                                      int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left,
                                                      int32_t pad_bottom, int32_t pad_right) {
    BackwardShape s;
    if (fill_shape(s, "conv_backward_workspace_bytes", batch, height, width, cin, cout, kh, kw, stride, pad_top, pad_left, pad_bottom,
                   pad_right))
        return 0;
    return backward_workspace_bytes(s);
}

extern "C" int32_t mrcnn_conv_backward_weights_chunk(int32_t batch, int32_t height, int32_t width, int32_t cin, int32_t cout,
                                                     int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left,
                                                     int32_t pad_bottom, int32_t pad_right) {
    BackwardShape s;
    if (fill_shape(s, "conv_backward_weights_chunk", batch, height, width, cin, cout, kh, kw, stride, pad_top, pad_left, pad_bottom,
                   pad_right))
        return 0;
    return wgrad_chunk(s.M, s.Cout, s.N);
}

extern "C" int mrcnn_conv_act_backward_f32(const float* dy, const float* y, int32_t batch, int32_t out_h, int32_t out_w, int32_t cout,
                                           const float* scale, int32_t activation, int32_t res_div, int32_t scatter,
                                           const int32_t* row_counts, int32_t rows_per_group, float* z, float* g, float* dresidual2,
                                           float* dshift, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream) {
    const char* who = "conv_act_backward";
    MRCNN_REQUIRE(activation >= 0 && activation <= 2, "%s: activation must be 0 (none), 1 (ReLU) or 2 (sigmoid)", who);
    MRCNN_REQUIRE(batch >= 1 && out_h >= 1 && out_w >= 1 && cout >= 1 && cout <= 0x7ffffff0, "%s: bad shape B=%d OH=%d OW=%d Cout=%d", who,
                  batch, out_h, out_w, cout);
    MRCNN_REQUIRE(res_div == 0 || res_div == 1 || res_div == 2, "%s: res_div must be 0 (no residual), 1 or 2", who);
    const bool res2 = res_div == 2;
    MRCNN_REQUIRE(!(res_div && (activation == 2 || scatter)), "%s: a residual cannot be combined with sigmoid or the deconv scatter", who);
    MRCNN_REQUIRE(!(scatter && activation == 2), "%s: deconv scatter supports activation 0 or 1", who);
    MRCNN_REQUIRE(!(scatter && cout % 4), "%s: the scatter's column count is 4 x the channels, got %d", who, cout);
    MRCNN_REQUIRE(!(scatter && g), "%s: g has no scattered form", who);
    MRCNN_REQUIRE(!res2 || (out_h % 2 == 0 && out_w % 2 == 0 && dresidual2), "%s: res_div=2 needs even output size and dresidual2", who);
    MRCNN_REQUIRE(res2 || !dresidual2, "%s: dresidual2 needs res_div=2", who);
    const long long M = 1LL * batch * out_h * out_w;
    const int C4 = (cout + 3) / 4 * 4;
    MRCNN_REQUIRE(4LL * M * C4 <= MAX_BUFFER_BYTES && M < (1LL << 31),
                  "%s: tensor too large (each tensor, z included, <= 0xFFFFFFF0 bytes: 32-bit buffer byte offsets)", who);
    if (row_counts) {
        MRCNN_REQUIRE(!res_div && !scatter, "%s: row counts cannot be combined with a residual or the deconv scatter", who);
        MRCNN_REQUIRE(rows_per_group >= 1 && M % rows_per_group == 0, "%s: %lld output rows are not whole groups of %d", who, M,
                      rows_per_group);
    }
    if (!z && !g && !dresidual2 && !dshift) return MRCNN_OK;
    MRCNN_REQUIRE(dy && (y || activation == 0), "%s: null pointer", who);
    const ActGeometry a = act_geometry(M, C4, res2);
    const size_t need = dshift ? sizeof(double) * static_cast<size_t>(a.blocks) * a.RT * C4 : 0;
    MRCNN_REQUIRE(!dshift || (workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 16 == 0),
                  "%s: workspace of %zu bytes, 16-byte aligned, needed (got %zu)", who, need, workspace_bytes);
    ActBackwardParams p;
    p.dy = dy; p.y = y; p.scale = scale; p.row_counts = row_counts; p.z = z; p.g = g; p.dres2 = dresidual2;
    p.part = dshift ? static_cast<double*>(workspace) : nullptr;
    p.M = static_cast<int>(M); p.OH = out_h; p.OW = out_w; p.C = cout; p.C4 = C4; p.act = activation; p.scatter = scatter ? 1 : 0;
    p.rows_per_group = row_counts ? rows_per_group : 1;
    p.units = a.units; p.units_per_block = a.units_per_block; p.CT = a.CT; p.RT = a.RT;
    hipStream_t s = mrcnn::as_stream(stream);
    if (res2) hipLaunchKernelGGL(conv_act_backward<true>, dim3(a.blocks), dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL(conv_act_backward<false>, dim3(a.blocks), dim3(kThreads), 0, s, p);
    if (int rc = mrcnn::check_launch("conv_act_backward")) return rc;
    if (dshift) return launch_reduce(p.part, C4, a.blocks * a.RT, cout, dshift, s);
    return MRCNN_OK;
}

extern "C" int mrcnn_conv_backward_data_f32(const float* z, int32_t batch, int32_t height, int32_t width, int32_t cin, const float* w,
                                            int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left,
                                            int32_t pad_bottom, int32_t pad_right, float* dx, void* workspace, size_t workspace_bytes,
                                            mrcnn_stream_t stream) {
    const char* who = "conv_backward_data";
    BackwardShape s;
    if (int rc = fill_shape(s, who, batch, height, width, cin, cout, kh, kw, stride, pad_top, pad_left, pad_bottom, pad_right)) return rc;
    MRCNN_REQUIRE(stride == 1 || (kh == 1 && kw == 1 && pad_top == 0 && pad_left == 0 && pad_bottom == 0 && pad_right == 0),
                  "%s: the stride-2 data gradient covers the 1 x 1 kernel without padding, got %d x %d with pads (%d, %d, %d, %d)", who,
                  kh, kw, pad_top, pad_left, pad_bottom, pad_right);
    MRCNN_REQUIRE(z && w && dx, "%s: null pointer", who);
    const size_t need = sizeof(float) * static_cast<size_t>(s.N) * s.Cout4;
    MRCNN_REQUIRE(workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
                  "%s: workspace of %zu bytes, 16-byte aligned, needed (got %zu)", who, need, workspace_bytes);
    float* wt = static_cast<float*>(workspace);
    hipStream_t st = mrcnn::as_stream(stream);
    const long long total = s.N * s.Cout4;
    hipLaunchKernelGGL(conv_weight_flip, dim3(static_cast<unsigned>((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, w, cout,
                       s.Cout4, kh, kw, cin, wt);
    if (int rc = mrcnn::check_launch("conv_weight_flip")) return rc;
    // the forward at stride 1 on the output map: at stride 2 (1 x 1, pads 0) a plain GEMM that writes the compact [B][OH][OW][Cin]
    return mrcnn_conv_bn_act_nhwc_f32(z, batch, s.OH, s.OW, s.Cout4, wt, cin, kh, kw, 1, kh - 1 - pad_top, kw - 1 - pad_left,
                                      kh - 1 - pad_bottom, kw - 1 - pad_right, nullptr, nullptr, nullptr, 1, 0, dx, stream);
}

// The stride only moves the pixel table's (iy0, ix0) and, through M, the chunk length.
extern "C" int mrcnn_conv_backward_weights_f32(const float* x, int32_t batch, int32_t height, int32_t width, int32_t cin,
                                               const float* z, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top,
                                               int32_t pad_left, int32_t pad_bottom, int32_t pad_right, const int32_t* row_counts,
                                               int32_t rows_per_group, float* dw, void* workspace, size_t workspace_bytes,
                                               mrcnn_stream_t stream) {
    const char* who = "conv_backward_weights";
    BackwardShape s;
    if (int rc = fill_shape(s, who, batch, height, width, cin, cout, kh, kw, stride, pad_top, pad_left, pad_bottom, pad_right)) return rc;
    MRCNN_REQUIRE(!(row_counts && stride != 1), "%s: row counts need stride 1", who);
    MRCNN_REQUIRE(x && z && dw, "%s: null pointer", who);
    if (row_counts)
        MRCNN_REQUIRE(rows_per_group >= 1 && s.M % rows_per_group == 0, "%s: %lld output rows are not whole groups of %d", who, s.M,
                      rows_per_group);
    const size_t need = wgrad_partial_bytes(s);
    MRCNN_REQUIRE(workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 16 == 0,
                  "%s: workspace of %zu bytes, 16-byte aligned, needed (got %zu)", who, need, workspace_bytes);
    WgradParams p;
    p.x = x; p.z = z; p.part = static_cast<float*>(workspace); p.row_counts = row_counts;
    p.rows_per_group = row_counts ? rows_per_group : 1;
    p.H = height; p.W = width; p.Cin = cin; p.Cout = cout; p.Cout4 = s.Cout4; p.KW = kw; p.pad_t = pad_top; p.pad_l = pad_left;
    p.OH = s.OH; p.OW = s.OW; p.stride = stride; p.M = static_cast<int>(s.M); p.N = static_cast<int>(s.N);
    p.L = wgrad_chunk(s.M, cout, s.N);
    p.x_bytes = static_cast<unsigned>(4LL * batch * height * width * cin);
    p.z_bytes = static_cast<unsigned>(4LL * s.M * s.Cout4);
    const int chunks = static_cast<int>((s.M + p.L - 1) / p.L);
    hipStream_t st = mrcnn::as_stream(stream);
    const int bm = wgrad_bm(cout);
    if (int rc = bm == 32   ? launch_wgrad<32, 1, 4>(p, chunks, st)
                 : bm == 64 ? launch_wgrad<64, 1, 4>(p, chunks, st)
                            : launch_wgrad<128, 2, 2>(p, chunks, st))
        return rc;
    return launch_reduce(p.part, 1LL * cout * s.N, chunks, 1LL * cout * s.N, dw, st);
}
