// The five training losses of Mask R-CNN for a batch of images, forward and backward (gfx950): RPN.class_loss / RPN.boxes_loss
// (model.py:652-718), Classifier.class_loss / Classifier.boxes_loss (model.py:802-845) and Mask.mask_loss (model.py:922-953) on the
// padded [B, count, ...] outputs of the target kernels, read in place. The rule is stated at mrcnn_rpn_loss_forward in
// include/maskrcnn_hip.h: every term and derivative in fp64 from the fp32 inputs, sums by store-and-sum (a workgroup stores its
// partial, a later launch adds the partials in a fixed order; no floating-point atomic, no ticket), an element that does not
// contribute is never loaded.
#include <cmath>

#include "common.hpp"
#include "loss_math.hpp"
#include "workgroup.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / mrcnn::kWave;
constexpr int kItems = 4;
constexpr int kChunk = kBlock * kItems;      // anchors of one workgroup of the RPN kernels
constexpr int kFinish = 1024;                // threads of the RPN finishing workgroup, one per target row
constexpr int kMaxAnchors = 1 << 24, kMaxBatch = 65535, kMaxCount = 1024, kMaxClasses = 4096, kMaxMaskSide = 64;

// ---------------------------------------------------------------------------------------------------------------------------
// the per-element definitions: torch's cross_entropy, smooth_l1_loss (beta 1) and binary_cross_entropy, in fp64
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double smooth_l1(double d) {
    const double a = fabs(d);
    return a < 1.0 ? 0.5 * d * d : a - 0.5;
}

__device__ __forceinline__ double smooth_l1_grad(double d) { return fabs(d) < 1.0 ? d : (d > 0.0 ? 1.0 : -1.0); }

__device__ __forceinline__ double box_terms(float4 p, float4 t) {
    return ((smooth_l1((double)p.x - (double)t.x) + smooth_l1((double)p.y - (double)t.y)) + smooth_l1((double)p.z - (double)t.z)) +
           smooth_l1((double)p.w - (double)t.w);
}

__device__ __forceinline__ float4 box_grads(float4 p, float4 t, double scale) {
    return make_float4((float)(scale * smooth_l1_grad((double)p.x - (double)t.x)), (float)(scale * smooth_l1_grad((double)p.y - (double)t.y)),
                       (float)(scale * smooth_l1_grad((double)p.z - (double)t.z)), (float)(scale * smooth_l1_grad((double)p.w - (double)t.w)));
}

using mrcnn::bce_grad;   // binary cross entropy, its derivative and a slot's sum: loss_math.hpp, shared with mask_train.hip

// cross entropy over the RPN's two logits with class c: log(sum exp(x - max)) - (x[c] - max)
__device__ __forceinline__ double ce2(float2 x, int c) {
    const double x0 = x.x, x1 = x.y, m = fmax(x0, x1);
    return log(exp(x0 - m) + exp(x1 - m)) - ((c ? x1 : x0) - m);
}

// the scale of each loss's gradient for image b: loss_math.hpp's, at this file's workgroup size
template <int kLosses>
__device__ __forceinline__ void loss_scales(const int32_t* counts, const float* grad_out, int per_image, int batch, int b, long long* red,
                                            double* scale) {
    mrcnn::loss_scales<kLosses, kBlock>(counts, grad_out, per_image, batch, b, red, scale);
}

// ---------------------------------------------------------------------------------------------------------------------------
// RPN: positives are ranked in ascending anchor index, as mrcnn_rpn_deltas ranks them: per-chunk counts, summed over the chunks
// in front
// ---------------------------------------------------------------------------------------------------------------------------
struct ChunkRanks {
    int before[kItems];   // positives of the chunk in front of this thread's wave, for each of its items
    int total;
};

// s_pos[it][wave] = positives of that wave in pass `it`, written before the barrier the caller put in front of this
__device__ __forceinline__ ChunkRanks chunk_ranks(const int (*s_pos)[kWaves], int wave) {
    ChunkRanks r;
    int running = 0;
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w == wave) r.before[it] = running;
            running += s_pos[it][w];
        }
    }
    r.total = running;
    return r;
}

__device__ __forceinline__ int lanes_before(unsigned long long ballot, int lane) { return __popcll(ballot & ((1ull << lane) - 1ull)); }

// One workgroup per chunk of kChunk anchors: the chunk's class-loss partial, its counts, and the anchors of its first `cap`
// positives.
__global__ __launch_bounds__(kBlock) void rpn_loss_chunk_kernel(const int32_t* match, const float* logits, int a_count, int chunks, int cap,
                                                                 double* part, int32_t* chunk_pos, int32_t* chunk_nz, int32_t* list) {
    __shared__ int s_pos[kItems][kWaves];
    __shared__ int s_nz[kItems][kWaves];
    __shared__ double s_red[kWaves];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y, chunk = (int)blockIdx.x;
    const int lane = tid % mrcnn::kWave, wave = tid / mrcnn::kWave;
    const int64_t base = (int64_t)b * a_count;
    double acc = 0.0;
    unsigned long long ballots[kItems];
    bool on[kItems];
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int a = chunk * kChunk + it * kBlock + tid;
        const int m = a < a_count ? match[base + a] : 0;
        if (m != 0) acc += ce2(*reinterpret_cast<const float2*>(logits + 2 * (base + a)), m == 1);
        on[it] = m == 1;
        ballots[it] = __ballot(on[it]);
        const unsigned long long nz = __ballot(m != 0);
        if (lane == 0) {
            s_pos[it][wave] = __popcll(ballots[it]);
            s_nz[it][wave] = __popcll(nz);
        }
    }
    __syncthreads();
    const ChunkRanks r = chunk_ranks(s_pos, wave);
    const int64_t slot = (int64_t)b * chunks + chunk;
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int k = r.before[it] + lanes_before(ballots[it], lane);
        if (on[it] && k < cap) list[slot * cap + k] = chunk * kChunk + it * kBlock + tid;
    }
    int nz = 0;
    if (tid == 0) {
#pragma unroll
        for (int it = 0; it < kItems; ++it)
#pragma unroll
            for (int w = 0; w < kWaves; ++w) nz += s_nz[it][w];
    }
    const double total = mrcnn::block_sum<kBlock>(acc, s_red);
    if (tid == 0) {
        part[slot] = total;
        chunk_pos[slot] = r.total;
        chunk_nz[slot] = nz;
    }
}

// One workgroup per image: the chunk partials in chunk order, the positives' anchors by rank, one target row per thread.
__global__ __launch_bounds__(kFinish) void rpn_loss_finish_kernel(const float* pred, const float* target, int a_count, int chunks, int cap,
                                                                   int count, const double* part, const int32_t* chunk_pos,
                                                                   const int32_t* chunk_nz, const int32_t* list, double* sums,
                                                                   int32_t* counts, int32_t* status) {
    __shared__ int s_anchor[kMaxCount];
    __shared__ int s_ired[kFinish / mrcnn::kWave];
    __shared__ double s_dred[kFinish / mrcnn::kWave];
    const int t = (int)threadIdx.x, b = (int)blockIdx.x;
    const int per = (chunks + kFinish - 1) / kFinish;
    const int lo = min(t * per, chunks), hi = min(lo + per, chunks);
    const int64_t row = (int64_t)b * chunks;
    int np = 0, nz = 0;
    double cls = 0.0;
    for (int c = lo; c < hi; ++c) {
        np += chunk_pos[row + c];
        nz += chunk_nz[row + c];
        cls += part[row + c];
    }
    int total_pos;
    int rank = mrcnn::block_inclusive_scan<kFinish>(np, s_ired, total_pos) - np;
    for (int c = lo; c < hi && rank < count; ++c) {
        const int n = chunk_pos[row + c];
        for (int k = 0; k < min(n, cap) && rank + k < count; ++k) s_anchor[rank + k] = list[(row + c) * cap + k];
        rank += n;
    }
    const int total_nz = mrcnn::block_sum<kFinish>(nz, s_ired);       // its first barrier publishes s_anchor
    const double total_cls = mrcnn::block_sum<kFinish>(cls, s_dred);
    const int used = min(total_pos, count);
    double box = 0.0;
    if (t < used) {
        const int a = s_anchor[t];
        if (a >= 0 && a < a_count)
            box = box_terms(*reinterpret_cast<const float4*>(pred + 4 * ((int64_t)b * a_count + a)),
                            *reinterpret_cast<const float4*>(target + 4 * ((int64_t)b * count + t)));
    }
    const double total_box = mrcnn::block_sum<kFinish>(box, s_dred);
    if (t == 0) {
        sums[2 * (int64_t)b] = total_cls;
        sums[2 * (int64_t)b + 1] = total_box;
        counts[2 * (int64_t)b] = total_nz;
        counts[2 * (int64_t)b + 1] = 4 * used;
        status[b] = total_pos > count ? 1 : 0;
    }
}

struct RpnBackwardParams {
    const int32_t* match;
    const float* logits;
    const float* pred;
    const float* target;
    const int32_t* chunk_pos;
    const int32_t* counts;
    const float* grad_out;
    float* grad_logits;
    float* grad_bbox;
    int32_t a, chunks, count, batch, per_image;
};

__global__ __launch_bounds__(kBlock) void rpn_loss_backward_kernel(RpnBackwardParams p) {
    __shared__ int s_pos[kItems][kWaves];
    __shared__ int s_ired[kWaves];
    __shared__ long long s_lred[kWaves];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y, chunk = (int)blockIdx.x;
    const int lane = tid % mrcnn::kWave, wave = tid / mrcnn::kWave;
    const int64_t base = (int64_t)b * p.a;
    double scale[2];
    loss_scales<2>(p.counts, p.grad_out, p.per_image, p.batch, b, s_lred, scale);
    int before = 0;
    for (int c = tid; c < chunk; c += kBlock) before += p.chunk_pos[(int64_t)b * p.chunks + c];
    const int first = mrcnn::block_sum<kBlock>(before, s_ired);
    int m[kItems];
    unsigned long long ballots[kItems];
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int a = chunk * kChunk + it * kBlock + tid;
        m[it] = a < p.a ? p.match[base + a] : 0;
        ballots[it] = __ballot(m[it] == 1);
        if (lane == 0) s_pos[it][wave] = __popcll(ballots[it]);
    }
    __syncthreads();
    const ChunkRanks r = chunk_ranks(s_pos, wave);
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int a = chunk * kChunk + it * kBlock + tid;
        if (a >= p.a) continue;
        float2 gl = make_float2(0.f, 0.f);
        float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m[it] != 0) {
            const float2 x = *reinterpret_cast<const float2*>(p.logits + 2 * (base + a));
            const double x0 = x.x, x1 = x.y, mx = fmax(x0, x1);
            const double e0 = exp(x0 - mx), e1 = exp(x1 - mx), s = e0 + e1;
            const bool fg = m[it] == 1;
            gl = make_float2((float)(scale[0] * (e0 / s - (fg ? 0.0 : 1.0))), (float)(scale[0] * (e1 / s - (fg ? 1.0 : 0.0))));
        }
        if (m[it] == 1) {
            const int k = first + r.before[it] + lanes_before(ballots[it], lane);
            if (k >= 0 && k < p.count)     // chunk_pos is the caller's memory: never follow it out of the target rows
                gb = box_grads(*reinterpret_cast<const float4*>(p.pred + 4 * (base + a)),
                               *reinterpret_cast<const float4*>(p.target + 4 * ((int64_t)b * p.count + k)), scale[1]);
        }
        *reinterpret_cast<float2*>(p.grad_logits + 2 * (base + a)) = gl;
        *reinterpret_cast<float4*>(p.grad_bbox + 4 * (base + a)) = gb;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// heads: one workgroup per slot
// ---------------------------------------------------------------------------------------------------------------------------
struct HeadParams {
    const int32_t* ids;
    const int32_t* num_rois;
    const float* target_deltas;
    const float* target_mask;
    const float* logits;
    const float* pred_bbox;
    const float* pred_masks;
    int32_t batch, count, classes, hw;
};

struct Slot {
    int64_t index;   // b * count + s
    int cls;
    bool use, pos, bad;   // in the class loss; in the box and mask losses; a class id outside 0 .. C-1
};

__device__ __forceinline__ Slot head_slot(const HeadParams& p, int b, int s) {
    Slot t;
    t.index = (int64_t)b * p.count + s;
    const bool valid = s < min(max(p.num_rois[b], 0), p.count);
    t.cls = valid ? p.ids[t.index] : 0;
    t.bad = valid && (t.cls < 0 || t.cls >= p.classes);
    t.use = valid && !t.bad;
    t.pos = t.use && t.cls > 0;
    return t;
}

// max and sum exp(x - max) of a slot's logits row; every thread of the workgroup
__device__ __forceinline__ void softmax_stats(const float* x, int classes, float* s_fred, double* s_dred, double& mx, double& sum) {
    float m = -INFINITY;
    for (int j = (int)threadIdx.x; j < classes; j += kBlock) m = fmaxf(m, x[j]);
    m = mrcnn::block_reduce<kBlock>(m, s_fred, [](float a, float c) { return fmaxf(a, c); });
    mx = (double)m;
    double e = 0.0;
    for (int j = (int)threadIdx.x; j < classes; j += kBlock) e += exp((double)x[j] - mx);
    sum = mrcnn::block_sum<kBlock>(e, s_dred);
}

__global__ __launch_bounds__(kBlock) void head_loss_slot_kernel(HeadParams p, double* part, int32_t* flags) {
    __shared__ float s_fred[kWaves];
    __shared__ double s_dred[kWaves];
    const int tid = (int)threadIdx.x;
    const Slot t = head_slot(p, (int)blockIdx.y, (int)blockIdx.x);    // the same in every thread: the branches below are uniform
    double ce = 0.0, box = 0.0, mask = 0.0;
    if (t.use) {
        const float* x = p.logits + t.index * p.classes;
        double mx, sum;
        softmax_stats(x, p.classes, s_fred, s_dred, mx, sum);
        ce = log(sum) - ((double)x[t.cls] - mx);
    }
    if (t.pos) {
        const int64_t plane = t.index * p.classes + t.cls;
        if (tid == 0)
            box = box_terms(*reinterpret_cast<const float4*>(p.pred_bbox + 4 * plane),
                            *reinterpret_cast<const float4*>(p.target_deltas + 4 * t.index));
        const float* pm = p.pred_masks + plane * p.hw;
        const float* tm = p.target_mask + t.index * p.hw;
        mask = mrcnn::bce_slot_sum<kBlock>(pm, tm, p.hw, s_dred);   // nothing is read when there is no mask tensor: hw is 0
    }
    if (tid == 0) {
        part[3 * t.index] = ce;
        part[3 * t.index + 1] = box;
        part[3 * t.index + 2] = mask;
        flags[t.index] = (t.use ? 1 : 0) | (t.pos ? 2 : 0) | (t.bad ? 4 : 0);
    }
}

// One workgroup per image: the slots' partials in slot order.
__global__ __launch_bounds__(kBlock) void head_loss_finish_kernel(const double* part, const int32_t* flags, int count, int hw, double* sums,
                                                                   int32_t* counts, int32_t* status) {
    __shared__ double s_part[3][kMaxCount];
    __shared__ int s_ired[kWaves];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    int n_cls = 0, n_pos = 0, n_bad = 0;
    for (int s = tid; s < count; s += kBlock) {
        const int64_t slot = (int64_t)b * count + s;
#pragma unroll
        for (int k = 0; k < 3; ++k) s_part[k][s] = part[3 * slot + k];
        const int f = flags[slot];
        n_cls += f & 1;
        n_pos += (f >> 1) & 1;
        n_bad += (f >> 2) & 1;
    }
    n_cls = mrcnn::block_sum<kBlock>(n_cls, s_ired);     // its first barrier publishes s_part
    n_pos = mrcnn::block_sum<kBlock>(n_pos, s_ired);
    n_bad = mrcnn::block_sum<kBlock>(n_bad, s_ired);
    if (tid < 3) {
        double acc = 0.0;
        for (int s = 0; s < count; ++s) acc += s_part[tid][s];
        sums[3 * (int64_t)b + tid] = acc;
    }
    if (tid == 0) {
        counts[3 * (int64_t)b] = n_cls;
        counts[3 * (int64_t)b + 1] = 4 * n_pos;
        counts[3 * (int64_t)b + 2] = n_pos * hw;
        status[b] = n_bad ? 2 : 0;
    }
}

struct HeadBackwardParams {
    HeadParams in;
    const int32_t* counts;
    const float* grad_out;
    float* grad_logits;
    float* grad_bbox;
    float* grad_masks;
    int32_t per_image;
};

__global__ __launch_bounds__(kBlock) void head_loss_backward_kernel(HeadBackwardParams q) {
    __shared__ float s_fred[kWaves];
    __shared__ double s_dred[kWaves];
    __shared__ long long s_lred[kWaves];
    const HeadParams& p = q.in;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const Slot t = head_slot(p, b, (int)blockIdx.x);
    double scale[3];
    loss_scales<3>(q.counts, q.grad_out, q.per_image, p.batch, b, s_lred, scale);
    // the logits row
    float* gl = q.grad_logits + t.index * p.classes;
    if (t.use) {
        const float* x = p.logits + t.index * p.classes;
        double mx, sum;
        softmax_stats(x, p.classes, s_fred, s_dred, mx, sum);
        for (int j = tid; j < p.classes; j += kBlock) gl[j] = (float)(scale[0] * (exp((double)x[j] - mx) / sum - (j == t.cls ? 1.0 : 0.0)));
    } else {
        for (int j = tid; j < p.classes; j += kBlock) gl[j] = 0.f;
    }
    // the box rows: zeros but the class's
    float4* gb = reinterpret_cast<float4*>(q.grad_bbox) + t.index * p.classes;
    for (int j = tid; j < p.classes; j += kBlock) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t.pos && j == t.cls)
            v = box_grads(*reinterpret_cast<const float4*>(p.pred_bbox + 4 * (t.index * p.classes + j)),
                          *reinterpret_cast<const float4*>(p.target_deltas + 4 * t.index), scale[1]);
        gb[j] = v;
    }
    // the mask planes: the slot's C * hw floats as one range, 16-byte stores between a scalar head and tail; [lo, hi) is the
    // class's plane (empty for a slot that does not contribute)
    const int total = p.classes * p.hw;
    const int lo = t.pos ? t.cls * p.hw : 0, hi = t.pos ? lo + p.hw : 0;
    float* gm = q.grad_masks + t.index * total;
    const float* pm = p.pred_masks + t.index * total;          // pm[i], i in [lo, hi)
    const float* tm = p.target_mask + t.index * p.hw - lo;     // tm[i], i in [lo, hi)
    auto value = [&](int i) -> float {
        return i >= lo && i < hi ? (float)(scale[2] * bce_grad((double)pm[i], (double)tm[i])) : 0.f;
    };
    const int head = min((int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(gm) & 15u)) & 15u) / 4u), total);
    const int vectors = (total - head) / 4;
    if (tid < head) gm[tid] = value(tid);
    for (int v = tid; v < vectors; v += kBlock) {
        const int i = head + 4 * v;
        float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i + 3 >= lo && i < hi) out = make_float4(value(i), value(i + 1), value(i + 2), value(i + 3));
        *reinterpret_cast<float4*>(gm + i) = out;
    }
    const int tail = head + 4 * vectors + tid;
    if (tid < 4 && tail < total) gm[tail] = value(tail);
}

// ---------------------------------------------------------------------------------------------------------------------------
// argument checks
// ---------------------------------------------------------------------------------------------------------------------------
int rpn_chunks(int32_t a) { return (a + kChunk - 1) / kChunk; }
int rpn_cap(int32_t count) { return count < kChunk ? count : kChunk; }

int check_batch(const char* who, int32_t batch, int32_t count) {
    MRCNN_REQUIRE(batch >= 1 && batch <= kMaxBatch, "%s: batch=%d must be in [1, %d]", who, batch, kMaxBatch);
    MRCNN_REQUIRE(count >= 1 && count <= kMaxCount, "%s: count=%d must be in [1, %d]", who, count, kMaxCount);
    return MRCNN_OK;
}

int check_rpn(const char* who, int32_t batch, int32_t a, int32_t count) {
    MRCNN_REQUIRE(a >= 1 && a <= kMaxAnchors, "%s: num_anchors=%d must be in [1, %d]", who, a, kMaxAnchors);
    if (int rc = check_batch(who, batch, count)) return rc;
    MRCNN_REQUIRE((int64_t)a * batch < (int64_t)1 << 31, "%s: batch * num_anchors = %lld is too large (must be < 2^31)", who,
                  (long long)((int64_t)a * batch));
    return MRCNN_OK;
}

int check_head(const char* who, int32_t batch, int32_t count, int32_t classes, int32_t mh, int32_t mw) {
    if (int rc = check_batch(who, batch, count)) return rc;
    MRCNN_REQUIRE(classes >= 2 && classes <= kMaxClasses, "%s: num_classes=%d must be in [2, %d]", who, classes, kMaxClasses);
    MRCNN_REQUIRE(mh >= 1 && mh <= kMaxMaskSide && mw >= 1 && mw <= kMaxMaskSide, "%s: mask_height=%d and mask_width=%d must be in [1, %d]",
                  who, mh, mw, kMaxMaskSide);
    return MRCNN_OK;
}

bool aligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

}  // namespace

extern "C" int32_t mrcnn_rpn_loss_chunks(int32_t num_anchors) { return num_anchors >= 1 && num_anchors <= kMaxAnchors ? rpn_chunks(num_anchors) : 0; }

extern "C" size_t mrcnn_rpn_loss_workspace_bytes(int32_t batch, int32_t num_anchors, int32_t count) {
    if (batch < 1 || num_anchors < 1 || num_anchors > kMaxAnchors || count < 1 || count > kMaxCount) return 0;
    return (size_t)batch * (size_t)rpn_chunks(num_anchors) * (sizeof(double) + sizeof(int32_t) * (1 + (size_t)rpn_cap(count)));
}

extern "C" int mrcnn_rpn_loss_forward(const int32_t* match, const float* logits, const float* pred_bbox, const float* target_bbox,
                                      int32_t batch, int32_t num_anchors, int32_t count, double* sums, int32_t* counts, int32_t* status,
                                      int32_t* chunk_pos, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream) {
    const char* who = "rpn_loss_forward";
    if (int rc = check_rpn(who, batch, num_anchors, count)) return rc;
    MRCNN_REQUIRE(match && logits && pred_bbox && target_bbox && sums && counts && status && chunk_pos && workspace, "%s: null pointer", who);
    MRCNN_REQUIRE(workspace_bytes >= mrcnn_rpn_loss_workspace_bytes(batch, num_anchors, count), "%s: workspace of %zu bytes, %zu needed", who,
                  workspace_bytes, mrcnn_rpn_loss_workspace_bytes(batch, num_anchors, count));
    MRCNN_REQUIRE(aligned(logits, 8) && aligned(pred_bbox, 16) && aligned(target_bbox, 16) && aligned(workspace, 8),
                  "%s: logits must be 8-byte aligned, pred_bbox and target_bbox 16-byte, the workspace 8-byte", who);
    const int chunks = rpn_chunks(num_anchors), cap = rpn_cap(count);
    const size_t slots = (size_t)batch * chunks;
    double* part = static_cast<double*>(workspace);
    int32_t* chunk_nz = reinterpret_cast<int32_t*>(part + slots);
    int32_t* list = chunk_nz + slots;
    hipStream_t s = mrcnn::as_stream(stream);
    hipLaunchKernelGGL(rpn_loss_chunk_kernel, dim3((unsigned)chunks, (unsigned)batch), dim3(kBlock), 0, s, match, logits, num_anchors, chunks,
                       cap, part, chunk_pos, chunk_nz, list);
    hipLaunchKernelGGL(rpn_loss_finish_kernel, dim3((unsigned)batch), dim3(kFinish), 0, s, pred_bbox, target_bbox, num_anchors, chunks, cap,
                       count, part, chunk_pos, chunk_nz, list, sums, counts, status);
    return mrcnn::check_launch(who);
}

extern "C" int mrcnn_rpn_loss_backward(const int32_t* match, const float* logits, const float* pred_bbox, const float* target_bbox,
                                       const int32_t* chunk_pos, const int32_t* counts, const float* grad_out, int32_t per_image,
                                       int32_t batch, int32_t num_anchors, int32_t count, float* grad_logits, float* grad_bbox,
                                       mrcnn_stream_t stream) {
    const char* who = "rpn_loss_backward";
    if (int rc = check_rpn(who, batch, num_anchors, count)) return rc;
    MRCNN_REQUIRE(match && logits && pred_bbox && target_bbox && chunk_pos && counts && grad_out && grad_logits && grad_bbox,
                  "%s: null pointer", who);
    MRCNN_REQUIRE(aligned(logits, 8) && aligned(grad_logits, 8) && aligned(pred_bbox, 16) && aligned(target_bbox, 16) && aligned(grad_bbox, 16),
                  "%s: logits and grad_logits must be 8-byte aligned, pred_bbox, target_bbox and grad_bbox 16-byte", who);
    RpnBackwardParams p;
    p.match = match; p.logits = logits; p.pred = pred_bbox; p.target = target_bbox; p.chunk_pos = chunk_pos; p.counts = counts;
    p.grad_out = grad_out; p.grad_logits = grad_logits; p.grad_bbox = grad_bbox;
    p.a = num_anchors; p.chunks = rpn_chunks(num_anchors); p.count = count; p.batch = batch; p.per_image = per_image != 0;
    hipLaunchKernelGGL(rpn_loss_backward_kernel, dim3((unsigned)p.chunks, (unsigned)batch), dim3(kBlock), 0, mrcnn::as_stream(stream), p);
    return mrcnn::check_launch(who);
}

extern "C" size_t mrcnn_head_loss_workspace_bytes(int32_t batch, int32_t count) {
    if (batch < 1 || count < 1 || count > kMaxCount) return 0;
    return (size_t)batch * (size_t)count * (3 * sizeof(double) + sizeof(int32_t));
}

namespace {
int head_params(const char* who, HeadParams& p, const int32_t* ids, const int32_t* num_rois, const float* target_deltas, const float* target_mask,
                const float* logits, const float* pred_bbox, const float* pred_masks, int32_t batch, int32_t count, int32_t classes, int32_t mh,
                int32_t mw) {
    if (int rc = check_head(who, batch, count, classes, mh, mw)) return rc;
    MRCNN_REQUIRE(ids && num_rois && target_deltas && logits && pred_bbox, "%s: null pointer", who);
    MRCNN_REQUIRE((target_mask != nullptr) == (pred_masks != nullptr), "%s: null pointer (target_mask and pred_masks are given together or both null)", who);
    MRCNN_REQUIRE(aligned(target_deltas, 16) && aligned(pred_bbox, 16), "%s: target_deltas and pred_bbox must be 16-byte aligned", who);
    p.ids = ids; p.num_rois = num_rois; p.target_deltas = target_deltas; p.target_mask = target_mask; p.logits = logits;
    p.pred_bbox = pred_bbox; p.pred_masks = pred_masks;
    p.batch = batch; p.count = count; p.classes = classes;
    p.hw = pred_masks ? mh * mw : 0;   // without the mask tensors: no mask term is read, the mask sum and count are 0, no gradient is written
    return MRCNN_OK;
}
}  // namespace

extern "C" int mrcnn_head_loss_forward(const int32_t* target_class_ids, const int32_t* num_rois, const float* target_deltas,
                                       const float* target_mask, const float* logits, const float* pred_bbox, const float* pred_masks,
                                       int32_t batch, int32_t count, int32_t num_classes, int32_t mask_height, int32_t mask_width,
                                       double* sums, int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes,
                                       mrcnn_stream_t stream) {
    const char* who = "head_loss_forward";
    HeadParams p;
    if (int rc = head_params(who, p, target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks, batch, count,
                             num_classes, mask_height, mask_width))
        return rc;
    MRCNN_REQUIRE(sums && counts && status && workspace, "%s: null pointer", who);
    MRCNN_REQUIRE(workspace_bytes >= mrcnn_head_loss_workspace_bytes(batch, count), "%s: workspace of %zu bytes, %zu needed", who,
                  workspace_bytes, mrcnn_head_loss_workspace_bytes(batch, count));
    MRCNN_REQUIRE(aligned(workspace, 8), "%s: the workspace must be 8-byte aligned", who);
    double* part = static_cast<double*>(workspace);
    int32_t* flags = reinterpret_cast<int32_t*>(part + 3 * (size_t)batch * count);
    hipStream_t s = mrcnn::as_stream(stream);
    hipLaunchKernelGGL(head_loss_slot_kernel, dim3((unsigned)count, (unsigned)batch), dim3(kBlock), 0, s, p, part, flags);
    hipLaunchKernelGGL(head_loss_finish_kernel, dim3((unsigned)batch), dim3(kBlock), 0, s, part, flags, count, p.hw, sums, counts, status);
    return mrcnn::check_launch(who);
}

extern "C" int mrcnn_head_loss_backward(const int32_t* target_class_ids, const int32_t* num_rois, const float* target_deltas,
                                        const float* target_mask, const float* logits, const float* pred_bbox, const float* pred_masks,
                                        const int32_t* counts, const float* grad_out, int32_t per_image, int32_t batch, int32_t count,
                                        int32_t num_classes, int32_t mask_height, int32_t mask_width, float* grad_logits, float* grad_bbox,
                                        float* grad_masks, mrcnn_stream_t stream) {
    const char* who = "head_loss_backward";
    HeadBackwardParams q;
    if (int rc = head_params(who, q.in, target_class_ids, num_rois, target_deltas, target_mask, logits, pred_bbox, pred_masks, batch, count,
                             num_classes, mask_height, mask_width))
        return rc;
    MRCNN_REQUIRE(counts && grad_out && grad_logits && grad_bbox, "%s: null pointer", who);
    MRCNN_REQUIRE((grad_masks != nullptr) == (pred_masks != nullptr), "%s: null pointer (grad_masks is given with pred_masks and null without)", who);
    MRCNN_REQUIRE(aligned(grad_bbox, 16) && aligned(grad_masks, 4), "%s: grad_bbox must be 16-byte aligned", who);
    q.counts = counts; q.grad_out = grad_out; q.grad_logits = grad_logits; q.grad_bbox = grad_bbox; q.grad_masks = grad_masks;
    q.per_image = per_image != 0;
    hipLaunchKernelGGL(head_loss_backward_kernel, dim3((unsigned)count, (unsigned)batch), dim3(kBlock), 0, mrcnn::as_stream(stream), q);
    return mrcnn::check_launch(who);
}
