// The mask head's class-plane branch in training (gfx950): the 1x1 conv to each slot's OWN class, its backward, and the mask loss on
// those planes, forward and backward. The rules are stated at mrcnn_class_plane_conv_f32 in include/maskrcnn_hip.h.
//
// Mask.mask_loss (model.py:922-953) reads plane target_class_ids[b][s] of the positive slots and nothing else, so of conv5's C output
// planes one per slot is computed, and none for a slot that is not active.
//   conv forward   one workgroup per (chunk of 64 pixels, slot, image); a wave owns a pixel at a time: lane l holds the channels
//                  4 (l + 64 i) .. + 3, multiplies and adds them in fp64 and the 64 lane sums meet in an xor butterfly.
//   conv backward  the same grid: one pass over x writes dx and, per (slot, chunk), the fp64 partial sums of g x and of g into the
//                  workspace (store-and-sum); the finishing launch has the owner of (class, channel) add its class's slots in ascending
//                  (b, s), which every wave finds by ballots over the ids.
//   loss           one workgroup per slot stores the slot's sum (loss_math.hpp: the code of the dense mask loss), a second launch adds
//                  an image's slots in slot order; the backward is one launch.
// No floating-point atomic, no memset, no ticket: every output byte is written by the thread that owns it.
#pragma clang fp contract(off)

#include <cmath>

#include "common.hpp"
#include "loss_math.hpp"
#include "workgroup.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / mrcnn::kWave;
constexpr int kPixels = 64;          // pixels of a slot per workgroup: wave v takes pixels v, v + 4, .. of the chunk
constexpr int kMaxBatch = 65535, kMaxCount = 1024, kMaxClasses = 4096, kMaxSide = 64, kMaxCin = 4096;

struct Planes {
    const int32_t* ids;              // [batch][count], read with stride count
    const int32_t* num;              // [batch]
    int32_t batch, count, slots, classes, q;   // slots = P plane slots per image, q = mh * mw
};

// The class of plane slot (b, s), or -1 when it is not active. The same in every thread that asks for the same slot.
__device__ __forceinline__ int active_class(const Planes& p, int b, int s) {
    if (s >= min(min(max(p.num[b], 0), p.count), p.slots)) return -1;
    const int k = p.ids[(int64_t)b * p.count + s];
    return k > 0 && k < p.classes ? k : -1;
}

// status[b] by ONE wave: bit 1 (2) a class id outside 0 .. C-1 below num[b], bit 2 (4) a positive at or past P below num[b].
__device__ __forceinline__ void plane_status(const Planes& p, int b, int lane, int32_t* status) {
    const int n = min(max(p.num[b], 0), p.count);
    bool bad = false, over = false;
    for (int base = 0; base < n; base += mrcnn::kWave) {
        const int s = base + lane;
        const int k = s < n ? p.ids[(int64_t)b * p.count + s] : 0;
        bad = bad || k < 0 || k >= p.classes;
        over = over || (k > 0 && s >= p.slots);
    }
    const int word = (__ballot(bad) ? 2 : 0) | (__ballot(over) ? 4 : 0);
    if (lane == 0) status[b] = word;
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// sum over the 64 lanes, the same bits in every lane: v + partner at distance 32, 16, .. 1 (an fp64 add commutes)
__device__ __forceinline__ double lanes_sum(double v) {
#pragma unroll
    for (int d = mrcnn::kWave / 2; d > 0; d >>= 1) v = v + __shfl_xor(v, d);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the 1x1 conv to the slot's class
// ---------------------------------------------------------------------------------------------------------------------------
struct ConvParams {
    Planes in;
    const float4* x;                 // [S][q][cin4]
    const float4* w;                 // [C][cin4]
    const float* bias;               // [C] or null
    float* y;                        // [S][q]
    int32_t* status;
    int32_t cin4, act;
};

// grid = (chunks of kPixels pixels, P, batch), block = 256
__global__ __launch_bounds__(kBlock) void class_plane_conv_kernel(ConvParams p) {
    const int lane = (int)threadIdx.x & (mrcnn::kWave - 1), wave = (int)threadIdx.x / mrcnn::kWave;
    const int s = (int)blockIdx.y, b = (int)blockIdx.z;
    if (blockIdx.x == 0 && s == 0 && wave == 0) plane_status(p.in, b, lane, p.status);
    const int k = active_class(p.in, b, s);
    const int64_t slot = (int64_t)b * p.in.slots + s;
    const int q0 = (int)blockIdx.x * kPixels, q1 = min(q0 + kPixels, p.in.q);
    float* y = p.y + slot * p.in.q;
    if (k < 0) {
        for (int q = q0 + (int)threadIdx.x; q < q1; q += kBlock) y[q] = 0.f;
        return;
    }
    const float4* w = p.w + (int64_t)k * p.cin4;
    const float4 w0 = lane < p.cin4 ? w[lane] : zero4();      // the first 256 channels of the class's row stay in registers
    const double bias = p.bias ? (double)p.bias[k] : 0.0;
    for (int q = q0 + wave; q < q1; q += kWaves) {
        const float4* x = p.x + (slot * p.in.q + q) * p.cin4;
        double acc = 0.0;
        for (int g = lane, i = 0; g < p.cin4; g += mrcnn::kWave, ++i) {
            const float4 xv = x[g];
            const float4 wv = i == 0 ? w0 : w[g];
            acc = acc + (double)xv.x * (double)wv.x;
            acc = acc + (double)xv.y * (double)wv.y;
            acc = acc + (double)xv.z * (double)wv.z;
            acc = acc + (double)xv.w * (double)wv.w;
        }
        const double total = lanes_sum(acc);
        if (lane == 0) {
            const float z = (float)(p.bias ? bias + total : total);
            y[q] = p.act == 2 ? 1.0f / (1.0f + expf(-z)) : z;
        }
    }
}

struct ConvBackwardParams {
    Planes in;
    const float* dy;                 // [S][q]
    const float* y;                  // [S][q], read at act 2 only
    const float4* x;                 // [S][q][cin4], read for dw only
    const float4* w;
    float4* dx;                      // [S][q][cin4] or null
    double* part_w;                  // [S][chunks][cin] or null (dw not asked for)
    double* part_b;                  // [S][chunks] or null
    int32_t cin4, act, chunks;
};

// grid = (chunks, P, batch), block = 256. LDS: the partial sums of waves 1 .. 3 for one group of 256 channels.
__global__ __launch_bounds__(kBlock) void class_plane_backward_kernel(ConvBackwardParams p) {
    __shared__ double s_part[kWaves - 1][mrcnn::kWave][4];
    __shared__ double s_bias[kWaves - 1];
    const int lane = (int)threadIdx.x & (mrcnn::kWave - 1), wave = (int)threadIdx.x / mrcnn::kWave;
    const int s = (int)blockIdx.y, b = (int)blockIdx.z, chunk = (int)blockIdx.x;
    const int k = active_class(p.in, b, s);
    const int64_t slot = (int64_t)b * p.in.slots + s;
    const int q0 = chunk * kPixels, q1 = min(q0 + kPixels, p.in.q);
    if (k < 0) {                                  // workgroup-uniform: no barrier below is skipped by part of the workgroup
        if (p.dx) {
            float4* dx = p.dx + (slot * p.in.q + q0) * p.cin4;
            const int n = (q1 - q0) * p.cin4;
            for (int e = (int)threadIdx.x; e < n; e += kBlock) dx[e] = zero4();
        }
        return;
    }
    const float* dy = p.dy + slot * p.in.q;
    const float* y = p.y + slot * p.in.q;
    auto grad = [&](int q) -> float {             // conv_act_backward's rule: three separately rounded fp32 operations
        const float d = dy[q];
        if (p.act != 2) return d;
        const float v = y[q];
        const float t = 1.0f - v;
        const float u = v * t;
        return d * u;
    };
    const float4* w = p.w + (int64_t)k * p.cin4;
    const int64_t part = slot * p.chunks + chunk;
    if (p.part_b) {                               // wave v adds its pixels' g in ascending order; the waves in wave order
        double acc = 0.0;
        for (int q = q0 + wave; q < q1; q += kWaves) acc = acc + (double)grad(q);
        if (wave > 0 && lane == 0) s_bias[wave - 1] = acc;
        __syncthreads();
        if (wave == 0 && lane == 0) p.part_b[part] = ((acc + s_bias[0]) + s_bias[1]) + s_bias[2];
    }
    const int groups = (p.cin4 + mrcnn::kWave - 1) / mrcnn::kWave;
    for (int i = 0; i < groups; ++i) {            // 256 channels at a time: g is read again, x and dx once
        const int c4 = i * mrcnn::kWave + lane;
        const bool mine = c4 < p.cin4;
        const float4 wv = mine ? w[c4] : zero4();
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int q = q0 + wave; q < q1; q += kWaves) {
            const float g = grad(q);
            const int64_t at = (slot * p.in.q + q) * p.cin4 + c4;
            if (mine && p.dx) p.dx[at] = make_float4(g * wv.x, g * wv.y, g * wv.z, g * wv.w);
            if (mine && p.part_w) {
                const float4 xv = p.x[at];
                const double gd = (double)g;
                a0 = a0 + gd * (double)xv.x;
                a1 = a1 + gd * (double)xv.y;
                a2 = a2 + gd * (double)xv.z;
                a3 = a3 + gd * (double)xv.w;
            }
        }
        if (!p.part_w) continue;                  // uniform
        __syncthreads();                          // the previous group's s_part has been read
        if (wave > 0) {
            s_part[wave - 1][lane][0] = a0;
            s_part[wave - 1][lane][1] = a1;
            s_part[wave - 1][lane][2] = a2;
            s_part[wave - 1][lane][3] = a3;
        }
        __syncthreads();
        if (wave == 0 && mine) {
            double* out = p.part_w + part * (4 * (int64_t)p.cin4) + 4 * (int64_t)c4;
            out[0] = ((a0 + s_part[0][lane][0]) + s_part[1][lane][0]) + s_part[2][lane][0];
            out[1] = ((a1 + s_part[0][lane][1]) + s_part[1][lane][1]) + s_part[2][lane][1];
            out[2] = ((a2 + s_part[0][lane][2]) + s_part[1][lane][2]) + s_part[2][lane][2];
            out[3] = ((a3 + s_part[0][lane][3]) + s_part[1][lane][3]) + s_part[2][lane][3];
        }
    }
}

struct ConvFinishParams {
    Planes in;
    const double* part_w;
    const double* part_b;
    float* dw;                       // [C][cin] or null
    float* dbias;                    // [C] or null
    int32_t cin, chunks;
};

// grid = (ceil(cin / 256), C), block = 256: thread t owns (class, channel blockIdx.x * 256 + t), and of the first workgroup of a
// class thread 0 owns dbias[class]. No barrier: every wave ranks the slots for itself.
__global__ __launch_bounds__(kBlock) void class_plane_finish_kernel(ConvFinishParams p) {
    const int lane = (int)threadIdx.x & (mrcnn::kWave - 1);
    const int k = (int)blockIdx.y, c = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    const bool has_w = p.dw && c < p.cin, has_b = p.dbias && blockIdx.x == 0 && threadIdx.x == 0;
    const int total = p.in.batch * p.in.slots;    // at most 65535 * 1024 < 2^31
    double acc_w = 0.0, acc_b = 0.0;
    for (int base = 0; base < total; base += mrcnn::kWave) {
        const int slot = base + lane;
        int cls = -1;
        if (slot < total) {
            const int b = slot / p.in.slots;
            cls = active_class(p.in, b, slot - b * p.in.slots);
        }
        unsigned long long hits = __ballot(cls == k && k > 0);     // the slots of class k among these 64, bit j = slot base + j
        while (hits) {                                              // ascending (b, s); uniform over the wave
            const int j = __ffsll((long long)hits) - 1;
            hits &= hits - 1;
            const int64_t first = (int64_t)(base + j) * p.chunks;
            if (has_w) {
                double sum = 0.0;
                for (int ch = 0; ch < p.chunks; ++ch) sum = sum + p.part_w[(first + ch) * p.cin + c];
                acc_w = acc_w + sum;
            }
            if (has_b) {
                double sum = 0.0;
                for (int ch = 0; ch < p.chunks; ++ch) sum = sum + p.part_b[first + ch];
                acc_b = acc_b + sum;
            }
        }
    }
    if (has_w) p.dw[(int64_t)k * p.cin + c] = (float)acc_w;
    if (has_b) p.dbias[k] = (float)acc_b;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the mask loss on the class planes
// ---------------------------------------------------------------------------------------------------------------------------
struct LossParams {
    Planes in;
    const float* p;                  // [batch][P][q]
    const float* target;             // [batch][count][q]
};

// grid = (P, batch), block = 256
__global__ __launch_bounds__(kBlock) void plane_loss_slot_kernel(LossParams p, double* part, int32_t* flags, int32_t* status) {
    __shared__ double s_dred[kWaves];
    const int s = (int)blockIdx.x, b = (int)blockIdx.y;
    if (s == 0 && threadIdx.x < mrcnn::kWave) plane_status(p.in, b, (int)threadIdx.x, status);
    const bool on = active_class(p.in, b, s) > 0;      // workgroup-uniform
    const int64_t slot = (int64_t)b * p.in.slots + s;
    double sum = 0.0;
    if (on) sum = mrcnn::bce_slot_sum<kBlock>(p.p + slot * p.in.q, p.target + ((int64_t)b * p.in.count + s) * p.in.q, p.in.q, s_dred);
    if (threadIdx.x == 0) {
        part[slot] = sum;
        flags[slot] = on ? 1 : 0;
    }
}

// grid = batch, block = 256: an image's slot sums in slot order
__global__ __launch_bounds__(kBlock) void plane_loss_finish_kernel(const double* part, const int32_t* flags, int slots, int q, double* sums,
                                                                    int32_t* counts) {
    __shared__ double s_part[kMaxCount];
    __shared__ int s_ired[kWaves];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    int n = 0;
    for (int s = tid; s < slots; s += kBlock) {
        s_part[s] = part[(int64_t)b * slots + s];
        n += flags[(int64_t)b * slots + s];
    }
    n = mrcnn::block_sum<kBlock>(n, s_ired);            // its first barrier publishes s_part
    if (tid == 0) {
        double acc = 0.0;
        for (int s = 0; s < slots; ++s) acc += s_part[s];
        sums[b] = acc;
        counts[b] = n * q;
    }
}

struct LossBackwardParams {
    LossParams in;
    const int32_t* counts;
    const float* grad_out;
    float* grad_p;                   // [batch][P][q]
    int32_t per_image;
};

// grid = (P, batch), block = 256
__global__ __launch_bounds__(kBlock) void plane_loss_backward_kernel(LossBackwardParams r) {
    __shared__ long long s_lred[kWaves];
    const Planes& in = r.in.in;
    const int s = (int)blockIdx.x, b = (int)blockIdx.y;
    double scale[1];
    mrcnn::loss_scales<1, kBlock>(r.counts, r.grad_out, r.per_image, in.batch, b, s_lred, scale);
    const bool on = active_class(in, b, s) > 0;
    const int64_t slot = (int64_t)b * in.slots + s;
    float* g = r.grad_p + slot * in.q;
    const float* pm = r.in.p + slot * in.q;
    const float* tm = r.in.target + ((int64_t)b * in.count + s) * in.q;
    for (int i = (int)threadIdx.x; i < in.q; i += kBlock) g[i] = on ? (float)(scale[0] * mrcnn::bce_grad((double)pm[i], (double)tm[i])) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------------
// argument checks
// ---------------------------------------------------------------------------------------------------------------------------
bool aligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

int fill_planes(const char* who, Planes& p, const int32_t* ids, const int32_t* num, int32_t batch, int32_t count, int32_t slots,
                int32_t classes, int32_t mh, int32_t mw) {
    MRCNN_REQUIRE(batch >= 1 && batch <= kMaxBatch, "%s: batch=%d must be in 1 .. %d", who, batch, kMaxBatch);
    MRCNN_REQUIRE(count >= 1 && count <= kMaxCount, "%s: count=%d must be in 1 .. %d", who, count, kMaxCount);
    MRCNN_REQUIRE(slots >= 1 && slots <= count, "%s: plane_slots=%d must be in 1 .. count = %d", who, slots, count);
    MRCNN_REQUIRE(classes >= 2 && classes <= kMaxClasses, "%s: num_classes=%d must be in 2 .. %d", who, classes, kMaxClasses);
    MRCNN_REQUIRE(mh >= 1 && mh <= kMaxSide && mw >= 1 && mw <= kMaxSide, "%s: mask_height=%d and mask_width=%d must be in 1 .. %d", who,
                  mh, mw, kMaxSide);
    MRCNN_REQUIRE(ids && num, "%s: null pointer", who);
    p.ids = ids; p.num = num; p.batch = batch; p.count = count; p.slots = slots; p.classes = classes; p.q = mh * mw;
    return MRCNN_OK;
}

int check_cin(const char* who, int32_t cin) {
    MRCNN_REQUIRE(cin >= 4 && cin <= kMaxCin && cin % 4 == 0, "%s: cin=%d must be a multiple of 4 in 4 .. %d", who, cin, kMaxCin);
    return MRCNN_OK;
}

int chunks_of(int q) { return (q + kPixels - 1) / kPixels; }

}  // namespace

extern "C" int mrcnn_class_plane_conv_f32(const float* x, const float* w, const float* bias, const int32_t* ids, const int32_t* num,
                                          int32_t batch, int32_t count, int32_t plane_slots, int32_t num_classes, int32_t mask_height,
                                          int32_t mask_width, int32_t cin, int32_t act, float* y, int32_t* status, mrcnn_stream_t stream) {
    const char* who = "class_plane_conv";
    ConvParams p;
    if (int rc = fill_planes(who, p.in, ids, num, batch, count, plane_slots, num_classes, mask_height, mask_width)) return rc;
    if (int rc = check_cin(who, cin)) return rc;
    MRCNN_REQUIRE(act == 0 || act == 2, "%s: act=%d must be 0 (none) or 2 (sigmoid)", who, act);
    MRCNN_REQUIRE(x && w && y && status, "%s: null pointer", who);
    MRCNN_REQUIRE(aligned(x, 16) && aligned(w, 16), "%s: x and w must be 16-byte aligned", who);
    p.x = reinterpret_cast<const float4*>(x); p.w = reinterpret_cast<const float4*>(w); p.bias = bias; p.y = y; p.status = status;
    p.cin4 = cin / 4; p.act = act;
    hipLaunchKernelGGL(class_plane_conv_kernel, dim3((unsigned)chunks_of(p.in.q), (unsigned)plane_slots, (unsigned)batch), dim3(kBlock), 0,
                       mrcnn::as_stream(stream), p);
    return mrcnn::check_launch("class_plane_conv_kernel");
}

extern "C" size_t mrcnn_class_plane_conv_backward_workspace_bytes(int32_t batch, int32_t plane_slots, int32_t mask_height,
                                                                  int32_t mask_width, int32_t cin) {
    if (batch < 1 || batch > kMaxBatch || plane_slots < 1 || plane_slots > kMaxCount || mask_height < 1 || mask_height > kMaxSide ||
        mask_width < 1 || mask_width > kMaxSide || cin < 4 || cin > kMaxCin)
        return 0;
    return (size_t)batch * plane_slots * chunks_of(mask_height * mask_width) * ((size_t)cin + 1) * sizeof(double);
}

extern "C" int mrcnn_class_plane_conv_backward_f32(const float* dy, const float* y, const float* x, const float* w, const int32_t* ids,
                                                   const int32_t* num, int32_t batch, int32_t count, int32_t plane_slots,
                                                   int32_t num_classes, int32_t mask_height, int32_t mask_width, int32_t cin, int32_t act,
                                                   float* dx, float* dw, float* dbias, void* workspace, size_t workspace_bytes,
                                                   mrcnn_stream_t stream) {
    const char* who = "class_plane_conv_backward";
    ConvBackwardParams p;
    if (int rc = fill_planes(who, p.in, ids, num, batch, count, plane_slots, num_classes, mask_height, mask_width)) return rc;
    if (int rc = check_cin(who, cin)) return rc;
    MRCNN_REQUIRE(act == 0 || act == 2, "%s: act=%d must be 0 (none) or 2 (sigmoid)", who, act);
    MRCNN_REQUIRE(dy && w && (y || act == 0) && (x || !dw), "%s: null pointer", who);
    MRCNN_REQUIRE(aligned(x, 16) && aligned(w, 16) && aligned(dx, 16), "%s: x, w and dx must be 16-byte aligned", who);
    if (!dx && !dw && !dbias) return MRCNN_OK;
    const size_t need = dw || dbias ? mrcnn_class_plane_conv_backward_workspace_bytes(batch, plane_slots, mask_height, mask_width, cin) : 0;
    MRCNN_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && aligned(workspace, 8)),
                  "%s: an 8-byte aligned workspace of %zu bytes is needed, %zu given", who, need, workspace_bytes);
    p.dy = dy; p.y = y; p.x = reinterpret_cast<const float4*>(x); p.w = reinterpret_cast<const float4*>(w);
    p.dx = reinterpret_cast<float4*>(dx);
    p.cin4 = cin / 4; p.act = act; p.chunks = chunks_of(p.in.q);
    const size_t parts = (size_t)batch * plane_slots * p.chunks;
    p.part_w = dw ? static_cast<double*>(workspace) : nullptr;
    p.part_b = dbias ? static_cast<double*>(workspace) + parts * cin : nullptr;
    hipStream_t s = mrcnn::as_stream(stream);
    hipLaunchKernelGGL(class_plane_backward_kernel, dim3((unsigned)p.chunks, (unsigned)plane_slots, (unsigned)batch), dim3(kBlock), 0, s, p);
    if (dw || dbias) {
        ConvFinishParams f;
        f.in = p.in; f.part_w = p.part_w; f.part_b = p.part_b; f.dw = dw; f.dbias = dbias; f.cin = cin; f.chunks = p.chunks;
        hipLaunchKernelGGL(class_plane_finish_kernel, dim3((unsigned)((cin + kBlock - 1) / kBlock), (unsigned)num_classes), dim3(kBlock), 0, s, f);
    }
    return mrcnn::check_launch(who);
}

extern "C" size_t mrcnn_mask_plane_loss_workspace_bytes(int32_t batch, int32_t plane_slots) {
    if (batch < 1 || batch > kMaxBatch || plane_slots < 1 || plane_slots > kMaxCount) return 0;
    return (size_t)batch * plane_slots * (sizeof(double) + sizeof(int32_t));
}

extern "C" int mrcnn_mask_plane_loss_forward(const float* p, const float* target_mask, const int32_t* ids, const int32_t* num,
                                             int32_t batch, int32_t count, int32_t plane_slots, int32_t num_classes, int32_t mask_height,
                                             int32_t mask_width, double* sums, int32_t* counts, int32_t* status, void* workspace,
                                             size_t workspace_bytes, mrcnn_stream_t stream) {
    const char* who = "mask_plane_loss_forward";
    LossParams q;
    if (int rc = fill_planes(who, q.in, ids, num, batch, count, plane_slots, num_classes, mask_height, mask_width)) return rc;
    MRCNN_REQUIRE(p && target_mask && sums && counts && status && workspace, "%s: null pointer", who);
    MRCNN_REQUIRE(workspace_bytes >= mrcnn_mask_plane_loss_workspace_bytes(batch, plane_slots) && aligned(workspace, 8),
                  "%s: an 8-byte aligned workspace of %zu bytes is needed, %zu given", who,
                  mrcnn_mask_plane_loss_workspace_bytes(batch, plane_slots), workspace_bytes);
    q.p = p; q.target = target_mask;
    double* part = static_cast<double*>(workspace);
    int32_t* flags = reinterpret_cast<int32_t*>(part + (size_t)batch * plane_slots);
    hipStream_t s = mrcnn::as_stream(stream);
    hipLaunchKernelGGL(plane_loss_slot_kernel, dim3((unsigned)plane_slots, (unsigned)batch), dim3(kBlock), 0, s, q, part, flags, status);
    hipLaunchKernelGGL(plane_loss_finish_kernel, dim3((unsigned)batch), dim3(kBlock), 0, s, part, flags, plane_slots, q.in.q, sums, counts);
    return mrcnn::check_launch(who);
}

extern "C" int mrcnn_mask_plane_loss_backward(const float* p, const float* target_mask, const int32_t* ids, const int32_t* num,
                                              const int32_t* counts, const float* grad_out, int32_t per_image, int32_t batch,
                                              int32_t count, int32_t plane_slots, int32_t num_classes, int32_t mask_height,
                                              int32_t mask_width, float* grad_p, mrcnn_stream_t stream) {
    const char* who = "mask_plane_loss_backward";
    LossBackwardParams r;
    if (int rc = fill_planes(who, r.in.in, ids, num, batch, count, plane_slots, num_classes, mask_height, mask_width)) return rc;
    MRCNN_REQUIRE(p && target_mask && counts && grad_out && grad_p, "%s: null pointer", who);
    r.in.p = p; r.in.target = target_mask; r.counts = counts; r.grad_out = grad_out; r.grad_p = grad_p; r.per_image = per_image != 0;
    hipLaunchKernelGGL(plane_loss_backward_kernel, dim3((unsigned)plane_slots, (unsigned)batch), dim3(kBlock), 0, mrcnn::as_stream(stream), r);
    return mrcnn::check_launch(who);
}
