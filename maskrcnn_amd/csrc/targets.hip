// RPN training targets: data.rpn_samples (data.py:449-591) for a batch of images, in three entry points.
//
//   mrcnn_anchor_match   steps 1-6 of the rule in include/maskrcnn_hip.h: fp32 IoU of every anchor against every row of every image,
//                        the row argmax / max and the crowd rule (target_match.hpp, shared with csrc/detection_targets.hip), the
//                        thresholds, and the column argmax (the forced positives).
//   mrcnn_sample_by_key  steps 7-8: of the positives (negatives) of an image the ones with the smallest (key, anchor index) are kept.
//   mrcnn_rpn_deltas     step 9: the positives' regression deltas in ascending anchor index, NumPy >= 2 promotion (fp32 box
//                        centre / size, fp64 anchor side, fp64 division and log, fp64 std-dev, narrowed to fp32 at the end).
//
// anchor_match. A thread owns ONE anchor and keeps its narrowed corners and area in registers for all B images; a workgroup
// stages an image's rows (box, area, class id) in LDS, 32 KB at the 1024-row limit. The column argmax crosses workgroups: a
// row's packed key is (IoU bits << 32 | ~anchor index): IoU >= +0, so its bit pattern is monotone, and of equal IoUs the smaller
// index has the larger key. A wave reduces its IoUs with a row by shuffles, its first lane at the maximum does ONE LDS atomic max
// (none where no lane of the wave touches the box), and after the row loop one global atomic max per (workgroup, row that was
// touched) merges the workgroups. A column whose IoUs are all zero needs no atomic at all: the key
// every kept row starts from IS (IoU 0, anchor 0), np.argmax's answer for an all-zero column. A maximum does not depend on the
// order of its operands, so the result is the same from run to run. The launch that needs every workgroup's maxima
// (forced_positive_kernel) is a separate launch: no flags, no spin waits.
//
// sample_by_key. The (key, anchor index) pairs of an image are distinct 55-bit numbers (31 key bits, 24 index bits), so "the k
// smallest" is "those <= the k-th smallest", and that one is found by a radix select: seven histogram passes of 8 bits from the
// top, positives and negatives in the same pass. A pass's workgroups first work out, each for itself and all alike, which digit
// the pass before has settled (a 256-bin scan of that pass's histogram: block_inclusive_scan, workgroup.hpp), then count the next digit of the elements that still
// carry the prefix: LDS histogram, then one integer atomic add per non-empty bin. Equal keys are told apart by the index bits, so
// any number of ties costs nothing extra. 1 memset + 7 passes + 1 marking launch, whatever B is (an image is a grid row).
//
// rpn_deltas. Row ix of an image's output is the ix-th positive in anchor order: a count per 4096-anchor chunk, then every
// chunk's workgroup sums the counts before it and ranks its own positives with wave ballots. 1 memset + 2 launches.
//
// Every index is checked where it is used: row offsets are clamped into [0, num_rows] and to 1024 rows an image, iou_argmax is
// compared with the image's row count, a decoded anchor index with A. Nothing here synchronises with the host.
#include "common.hpp"
#include "target_match.hpp"
#include "workgroup.hpp"

namespace {

using namespace mrcnn_match;

constexpr int kBlock = 256;
constexpr int kMaxAnchors = 1 << 24;       // index bits of the packed sampling key
constexpr int kPasses = 7;                 // 8-bit digits of the 56-bit (key << 24 | index)
constexpr int kSampleItems = 8;            // anchors per thread in a sampling pass
constexpr int kDeltaItems = 16;            // anchors per thread in the delta launches
constexpr int kDeltaChunk = kBlock * kDeltaItems;
constexpr unsigned long long kKeptInit = 0xffffffffull;   // (IoU +0, anchor 0); 0 = not a kept row

// ---------------------------------------------------------------------------------------------------------------------------
// anchor_match
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void match_init_kernel(const int32_t* ids, const int32_t* gt_off, int m,
                                                            unsigned long long* colkey, int32_t* status) {
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const Rows r = image_rows(gt_off, b, m);
    int crowd = 0;
    for (int i = tid; i < r.n; i += kBlock) crowd |= ids[r.start + i] < 0;
    crowd = __syncthreads_or(crowd);
    int kept = 0;
    for (int i = tid; i < r.n; i += kBlock) {
        const bool k = row_kept(ids[r.start + i], crowd != 0);
        colkey[r.start + i] = k ? kKeptInit : 0ull;
        kept |= k;
    }
    kept = __syncthreads_or(kept);
    if (tid == 0) status[b] = kept ? 0 : 1;
}

struct MatchParams {
    const double* anchors;
    const float* boxes;
    const int32_t* ids;
    const int32_t* gt_off;
    int32_t a, m, batch;
    float neg, pos, crowd;
    int32_t* match;
    int32_t* argmax;
    float* iou_max;
    unsigned long long* colkey;
};

__global__ __launch_bounds__(kBlock) void anchor_match_kernel(MatchParams p) {
    __shared__ float4 s_box[kMaxRows];
    __shared__ float s_area[kMaxRows];
    __shared__ int s_id[kMaxRows];
    __shared__ unsigned long long s_key[kMaxRows];
    const int tid = (int)threadIdx.x;
    const int a = (int)blockIdx.x * kBlock + tid;
    const bool live = a < p.a;
    float4 anchor = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {   // .float(): round to nearest
        const double* an = p.anchors + 4 * (int64_t)a;
        anchor = make_float4((float)an[0], (float)an[1], (float)an[2], (float)an[3]);
    }
    const float a_area = box_area(anchor);
    const unsigned long long low = (unsigned long long)(~(uint32_t)a);
    const int lane = tid % mrcnn::kWave;

    for (int b = 0; b < p.batch; ++b) {
        const Rows r = image_rows(p.gt_off, b, p.m);
        __syncthreads();                                   // the image before has been read by every lane
        int crowd = 0;
        for (int i = tid; i < r.n; i += kBlock) {
            const float* g = p.boxes + 4 * (int64_t)(r.start + i);
            const float4 box = make_float4(g[0], g[1], g[2], g[3]);
            const int id = p.ids[r.start + i];
            s_box[i] = box;
            s_area[i] = box_area(box);
            s_id[i] = id;
            s_key[i] = 0ull;
            crowd |= id < 0;
        }
        crowd = __syncthreads_or(crowd);

        Match walk;
        for (int g = 0; g < r.n; ++g) {
            const float iou = box_iou(anchor, a_area, s_box[g], s_area[g]);
            const int id = s_id[g];
            if (row_kept(id, crowd != 0)) {
                walk.kept_row(g, iou);
                // the wave's largest IoU with this row, and its first lane (lanes are in anchor order): ONE LDS atomic per wave
                // and row, and none where no lane of the wave touches the box
                const float mine = live && iou > 0.f ? iou : 0.f;
                float top = mine;
#pragma unroll
                for (int off = mrcnn::kWave / 2; off > 0; off >>= 1) top = fmaxf(top, __shfl_xor(top, off));
                if (top > 0.f) {                           // the same for the whole wave
                    const unsigned long long at_top = __ballot(mine == top);
                    if (lane == __ffsll((long long)at_top) - 1)
                        atomicMax(&s_key[g], ((unsigned long long)__float_as_uint(mine) << 32) | low);
                }
            } else if (id < 0) {
                walk.crowd_row(iou);
            }
        }
        __syncthreads();
        for (int i = tid; i < r.n; i += kBlock) {
            const unsigned long long k = s_key[i];
            if (k != 0ull) atomicMax(&p.colkey[r.start + i], k);
        }
        if (live) {
            const int64_t o = (int64_t)b * p.a + a;
            int mt = 0;
            if (walk.arg >= 0) {
                if (walk.best >= p.pos) mt = 1;
                else if (walk.best < p.neg && walk.crowd_max < p.crowd) mt = -1;
            }
            p.match[o] = mt;
            p.argmax[o] = walk.arg;
            p.iou_max[o] = walk.arg >= 0 ? walk.best : 0.f;
        }
    }
}

// every kept row's best anchor becomes positive (data.py:536-537); after ALL workgroups of anchor_match_kernel
__global__ __launch_bounds__(kBlock) void forced_positive_kernel(const int32_t* gt_off, int m, int a_count,
                                                                 const unsigned long long* colkey, int32_t* match,
                                                                 int32_t* gt_argmax) {
    const int b = (int)blockIdx.x;
    const Rows r = image_rows(gt_off, b, m);
    for (int i = (int)threadIdx.x; i < r.n; i += kBlock) {
        const unsigned long long k = colkey[r.start + i];
        int best = -1;
        if (k != 0ull) {
            const uint32_t a = ~(uint32_t)(k & 0xffffffffull);
            if (a < (uint32_t)a_count) {
                best = (int)a;
                match[(int64_t)b * a_count + a] = 1;
            }
        }
        gt_argmax[r.start + i] = best;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// sample_by_key
// ---------------------------------------------------------------------------------------------------------------------------
struct SelState {
    unsigned long long prefix;   // the digits settled so far, most significant first
    int32_t k;                   // how many of the elements that carry the prefix are kept
    int32_t mode;                // 0: keep all (nothing to subsample), 1: selecting, 2: keep none
};

struct SampleParams {
    const int32_t* match;
    const int32_t* keys;
    int32_t* out;
    uint32_t* hist;     // [kPasses][batch][2][256]
    SelState* state;    // [kPasses + 1][batch][2]; entry p: the state pass p filters with
    int32_t a, batch, count;
};

__device__ __forceinline__ unsigned long long packed_key(int32_t key, int a) {
    return ((unsigned long long)((uint32_t)key & 0x7fffffffu) << 24) | (unsigned long long)(uint32_t)a;
}

// The states pass p (1..kPasses) filters with, from pass p-1's state and histogram: class 0 the positives, class 1 the negatives.
// Every workgroup of image b computes the same values.
__device__ void resolve_states(const SampleParams& q, int b, int p, SelState (&st)[2], uint32_t* s_scan, int* s_pick) {
    const int tid = (int)threadIdx.x;
    int npos = 0;
    for (int c = 0; c < 2; ++c) {
        const uint32_t* h = q.hist + (((int64_t)(p - 1) * q.batch + b) * 2 + c) * 256;
        const uint32_t v = h[tid];
        uint32_t total;
        const uint32_t incl = mrcnn::block_inclusive_scan<kBlock>(v, s_scan, total);
        SelState prev;
        if (p == 1) {
            int k;
            if (c == 0) {
                npos = (int)total;
                k = q.count / 2;
            } else {
                k = q.count - min(npos, q.count / 2);
            }
            prev.prefix = 0ull;
            prev.k = k;
            prev.mode = (int64_t)total <= (int64_t)k ? 0 : (k == 0 ? 2 : 1);
        } else {
            prev = q.state[((int64_t)(p - 1) * q.batch + b) * 2 + c];
        }
        if (tid == 0) {
            s_pick[0] = 0;
            s_pick[1] = 0;
        }
        __syncthreads();
        if (prev.mode == 1 && incl >= (uint32_t)prev.k && incl - v < (uint32_t)prev.k) {   // one thread: 1 <= k <= total
            s_pick[0] = tid;
            s_pick[1] = (int)(incl - v);
        }
        __syncthreads();
        if (prev.mode == 1) {
            st[c].prefix = (prev.prefix << 8) | (unsigned long long)s_pick[0];
            st[c].k = prev.k - s_pick[1];
            st[c].mode = 1;
        } else {
            st[c] = prev;
        }
    }
}

__global__ __launch_bounds__(kBlock) void sample_hist_kernel(SampleParams q, int p) {
    __shared__ uint32_t s_hist[2][256];
    __shared__ uint32_t s_scan[kBlock / mrcnn::kWave];
    __shared__ int s_pick[2];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    SelState st[2];
    if (p == 0) {
        st[0] = st[1] = SelState{0ull, 0, 1};
    } else {
        resolve_states(q, b, p, st, s_scan, s_pick);
        if (blockIdx.x == 0 && tid == 0) {
            q.state[((int64_t)p * q.batch + b) * 2] = st[0];
            q.state[((int64_t)p * q.batch + b) * 2 + 1] = st[1];
        }
    }
    s_hist[0][tid] = 0u;
    s_hist[1][tid] = 0u;
    __syncthreads();
    const int shift_prefix = 56 - 8 * p, shift_digit = 48 - 8 * p;
    const int64_t base = (int64_t)b * q.a;
#pragma unroll
    for (int it = 0; it < kSampleItems; ++it) {
        const int a = ((int)blockIdx.x * kSampleItems + it) * kBlock + tid;
        if (a >= q.a) continue;
        const int mt = q.match[base + a];
        const int c = mt == 1 ? 0 : (mt == -1 ? 1 : -1);
        if (c < 0 || st[c].mode != 1) continue;
        const unsigned long long key = packed_key(q.keys[base + a], a);
        if ((key >> shift_prefix) == st[c].prefix) atomicAdd(&s_hist[c][(int)((key >> shift_digit) & 255ull)], 1u);
    }
    __syncthreads();
    uint32_t* h = q.hist + (((int64_t)p * q.batch + b) * 2) * 256;
    for (int c = 0; c < 2; ++c) {
        const uint32_t v = s_hist[c][tid];
        if (v != 0u) atomicAdd(&h[c * 256 + tid], v);
    }
}

__global__ __launch_bounds__(kBlock) void sample_mark_kernel(SampleParams q) {
    __shared__ uint32_t s_scan[kBlock / mrcnn::kWave];
    __shared__ int s_pick[2];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    SelState st[2];
    resolve_states(q, b, kPasses, st, s_scan, s_pick);      // prefix: the k-th smallest packed key itself
    const int64_t base = (int64_t)b * q.a;
#pragma unroll
    for (int it = 0; it < kSampleItems; ++it) {
        const int a = ((int)blockIdx.x * kSampleItems + it) * kBlock + tid;
        if (a >= q.a) continue;
        int mt = q.match[base + a];
        const int c = mt == 1 ? 0 : (mt == -1 ? 1 : -1);
        if (c >= 0 && st[c].mode != 0) {
            const bool keep = st[c].mode == 1 && packed_key(q.keys[base + a], a) <= st[c].prefix;
            if (!keep) mt = 0;
        }
        q.out[base + a] = mt;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// rpn_deltas
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void positive_count_kernel(const int32_t* match, int a_count, int chunks, int32_t* counts) {
    __shared__ int s_total;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    if (tid == 0) s_total = 0;
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int it = 0; it < kDeltaItems; ++it) {
        const int a = (int)blockIdx.x * kDeltaChunk + it * kBlock + tid;
        if (a < a_count) n += match[(int64_t)b * a_count + a] == 1;
    }
    if (n != 0) atomicAdd(&s_total, n);
    __syncthreads();
    if (tid == 0) counts[(int64_t)b * chunks + blockIdx.x] = s_total;
}

struct DeltaParams {
    const double* anchors;
    const float* boxes;
    const int32_t* gt_off;
    const int32_t* match;
    const int32_t* argmax;
    const int32_t* counts;
    float* bbox;
    int32_t* num_pos;
    int32_t a, m, count, chunks;
    double std_dev[4];
};

__global__ __launch_bounds__(kBlock) void rpn_deltas_kernel(DeltaParams p) {
    __shared__ int s_base;
    __shared__ int s_wave[kBlock / mrcnn::kWave];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const int lane = tid % mrcnn::kWave, wave = tid / mrcnn::kWave;
    if (tid == 0) s_base = 0;
    __syncthreads();
    int before = 0;
    for (int c = tid; c < (int)blockIdx.x; c += kBlock) before += p.counts[(int64_t)b * p.chunks + c];
    if (before != 0) atomicAdd(&s_base, before);
    __syncthreads();
    int base = s_base;
    const Rows r = image_rows(p.gt_off, b, p.m);
    for (int it = 0; it < kDeltaItems; ++it) {
        const int a = (int)blockIdx.x * kDeltaChunk + it * kBlock + tid;
        const bool on = a < p.a && p.match[(int64_t)b * p.a + a] == 1;
        const unsigned long long ballot = __ballot(on);
        if (lane == 0) s_wave[wave] = __popcll(ballot);
        __syncthreads();
        int before_wave = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kBlock / mrcnn::kWave; ++w) {
            const int n = s_wave[w];
            before_wave += w < wave ? n : 0;
            total += n;
        }
        __syncthreads();
        const int ix = base + before_wave + __popcll(ballot & ((1ull << lane) - 1ull));
        base += total;
        if (!on || ix >= p.count) continue;
        float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
        const int g = p.argmax[(int64_t)b * p.a + a];
        if (g >= 0 && g < r.n) {
            const float* gt = p.boxes + 4 * (int64_t)(r.start + g);
            const double* an = p.anchors + 4 * (int64_t)a;
            // the box side and centre in fp32 (0.5 * float32 stays float32 under NumPy >= 2), the anchor's in fp64
            const float gt_h = gt[2] - gt[0], gt_w = gt[3] - gt[1];
            const float gt_cy = gt[0] + 0.5f * gt_h, gt_cx = gt[1] + 0.5f * gt_w;
            const double a_h = an[2] - an[0], a_w = an[3] - an[1];
            const double a_cy = an[0] + 0.5 * a_h, a_cx = an[1] + 0.5 * a_w;
            const double dy = ((double)gt_cy - a_cy) / a_h, dx = ((double)gt_cx - a_cx) / a_w;
            const double dh = log((double)gt_h / a_h), dw = log((double)gt_w / a_w);
            out = make_float4((float)(dy / p.std_dev[0]), (float)(dx / p.std_dev[1]), (float)(dh / p.std_dev[2]),
                              (float)(dw / p.std_dev[3]));
        }
        *reinterpret_cast<float4*>(p.bbox + 4 * ((int64_t)b * p.count + ix)) = out;
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) p.num_pos[b] = base;
}

int delta_chunks(int32_t a) { return (a + kDeltaChunk - 1) / kDeltaChunk; }

// the limits of an entry point: A, B, the packed rows (sample_by_key takes none) and A * B
int check_shape(const char* who, int32_t a, int32_t batch, int32_t num_rows = 0) {
    MRCNN_REQUIRE(a >= 1 && a <= kMaxAnchors, "%s: num_anchors=%d must be in [1, %d]", who, a, kMaxAnchors);
    if (int rc = check_rows(who, num_rows, batch)) return rc;
    MRCNN_REQUIRE((int64_t)a * batch < (int64_t)1 << 31, "%s: batch * num_anchors = %lld is too large (must be < 2^31)", who,
                  (long long)((int64_t)a * batch));
    return MRCNN_OK;
}

}  // namespace

extern "C" size_t mrcnn_anchor_match_workspace_bytes(int32_t num_rows) {
    return num_rows > 0 ? (size_t)num_rows * sizeof(unsigned long long) : 0;
}

extern "C" int mrcnn_anchor_match(const double* anchors, int32_t num_anchors, const float* gt_boxes, const int32_t* gt_class_ids,
                                  const int32_t* gt_off, int32_t num_rows, int32_t batch, float neg_iou, float pos_iou,
                                  float crowd_iou, int32_t* match, int32_t* iou_argmax, float* iou_max, int32_t* gt_argmax,
                                  int32_t* status, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream) {
    if (int rc = check_shape("anchor_match", num_anchors, batch, num_rows)) return rc;
    MRCNN_REQUIRE(anchors && gt_off && match && iou_argmax && iou_max && status, "anchor_match: null pointer");
    MRCNN_REQUIRE(num_rows == 0 || (gt_boxes && gt_class_ids && gt_argmax && workspace), "anchor_match: null pointer");
    MRCNN_REQUIRE(workspace_bytes >= mrcnn_anchor_match_workspace_bytes(num_rows), "anchor_match: workspace of %zu bytes, %zu needed",
                  workspace_bytes, mrcnn_anchor_match_workspace_bytes(num_rows));
    MRCNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "anchor_match: the workspace must be 8-byte aligned");
    hipStream_t s = mrcnn::as_stream(stream);
    unsigned long long* colkey = static_cast<unsigned long long*>(workspace);
    if (num_rows > 0) {
        // rows that belong to no image: not kept, gt_argmax -1
        hipError_t e = hipMemsetAsync(colkey, 0, (size_t)num_rows * sizeof(unsigned long long), s);
        if (e == hipSuccess) e = hipMemsetAsync(gt_argmax, 0xff, (size_t)num_rows * sizeof(int32_t), s);
        if (e != hipSuccess) return mrcnn::fail(MRCNN_ERR_LAUNCH, "anchor_match: hipMemsetAsync: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(match_init_kernel, dim3((unsigned)batch), dim3(kBlock), 0, s, gt_class_ids, gt_off, num_rows, colkey, status);
    MatchParams p;
    p.anchors = anchors; p.boxes = gt_boxes; p.ids = gt_class_ids; p.gt_off = gt_off;
    p.a = num_anchors; p.m = num_rows; p.batch = batch;
    p.neg = neg_iou; p.pos = pos_iou; p.crowd = crowd_iou;
    p.match = match; p.argmax = iou_argmax; p.iou_max = iou_max; p.colkey = colkey;
    hipLaunchKernelGGL(anchor_match_kernel, dim3((unsigned)((num_anchors + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, p);
    hipLaunchKernelGGL(forced_positive_kernel, dim3((unsigned)batch), dim3(kBlock), 0, s, gt_off, num_rows, num_anchors, colkey,
                       match, gt_argmax);
    return mrcnn::check_launch("anchor_match");
}

extern "C" size_t mrcnn_sample_by_key_workspace_bytes(int32_t batch) {
    if (batch < 1) return 0;
    return (size_t)batch * ((size_t)kPasses * 2 * 256 * sizeof(uint32_t) + (size_t)(kPasses + 1) * 2 * sizeof(SelState));
}

extern "C" int mrcnn_sample_by_key(const int32_t* match, const int32_t* keys, int32_t batch, int32_t num_anchors, int32_t count,
                                   int32_t* out, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream) {
    if (int rc = check_shape("sample_by_key", num_anchors, batch)) return rc;
    MRCNN_REQUIRE(count >= 1, "sample_by_key: count=%d must be >= 1", count);
    MRCNN_REQUIRE(match && keys && out && workspace, "sample_by_key: null pointer");
    MRCNN_REQUIRE(workspace_bytes >= mrcnn_sample_by_key_workspace_bytes(batch), "sample_by_key: workspace of %zu bytes, %zu needed",
                  workspace_bytes, mrcnn_sample_by_key_workspace_bytes(batch));
    MRCNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, "sample_by_key: the workspace must be 16-byte aligned");
    hipStream_t s = mrcnn::as_stream(stream);
    const size_t hist_bytes = (size_t)batch * kPasses * 2 * 256 * sizeof(uint32_t);
    hipError_t e = hipMemsetAsync(workspace, 0, hist_bytes, s);
    if (e != hipSuccess) return mrcnn::fail(MRCNN_ERR_LAUNCH, "sample_by_key: hipMemsetAsync: %s", hipGetErrorString(e));
    SampleParams q;
    q.match = match; q.keys = keys; q.out = out;
    q.hist = static_cast<uint32_t*>(workspace);
    q.state = reinterpret_cast<SelState*>(static_cast<char*>(workspace) + hist_bytes);
    q.a = num_anchors; q.batch = batch; q.count = count;
    const int per_block = kBlock * kSampleItems;
    const dim3 grid((unsigned)((num_anchors + per_block - 1) / per_block), (unsigned)batch);
    for (int p = 0; p < kPasses; ++p) hipLaunchKernelGGL(sample_hist_kernel, grid, dim3(kBlock), 0, s, q, p);
    hipLaunchKernelGGL(sample_mark_kernel, grid, dim3(kBlock), 0, s, q);
    return mrcnn::check_launch("sample_by_key");
}

extern "C" size_t mrcnn_rpn_deltas_workspace_bytes(int32_t batch, int32_t num_anchors) {
    if (batch < 1 || num_anchors < 1) return 0;
    return (size_t)batch * (size_t)delta_chunks(num_anchors) * sizeof(int32_t);
}

extern "C" int mrcnn_rpn_deltas(const double* anchors, int32_t num_anchors, const float* gt_boxes, const int32_t* gt_off,
                                int32_t num_rows, int32_t batch, const int32_t* match, const int32_t* iou_argmax, int32_t count,
                                const double std_dev[4], float* rpn_bbox, int32_t* num_pos, void* workspace, size_t workspace_bytes,
                                mrcnn_stream_t stream) {
    if (int rc = check_shape("rpn_deltas", num_anchors, batch, num_rows)) return rc;
    MRCNN_REQUIRE(count >= 1, "rpn_deltas: count=%d must be >= 1", count);
    MRCNN_REQUIRE((int64_t)count * batch < (int64_t)1 << 29, "rpn_deltas: batch * count = %lld is too large (must be < 2^29)",
                  (long long)((int64_t)count * batch));
    MRCNN_REQUIRE(anchors && gt_off && match && iou_argmax && std_dev && rpn_bbox && num_pos && workspace, "rpn_deltas: null pointer");
    MRCNN_REQUIRE(num_rows == 0 || gt_boxes, "rpn_deltas: null pointer");
    MRCNN_REQUIRE(workspace_bytes >= mrcnn_rpn_deltas_workspace_bytes(batch, num_anchors), "rpn_deltas: workspace of %zu bytes, %zu needed",
                  workspace_bytes, mrcnn_rpn_deltas_workspace_bytes(batch, num_anchors));
    MRCNN_REQUIRE((reinterpret_cast<uintptr_t>(rpn_bbox) & 15u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0,
                  "rpn_deltas: rpn_bbox must be 16-byte aligned and the workspace 4-byte aligned");
    hipStream_t s = mrcnn::as_stream(stream);
    hipError_t e = hipMemsetAsync(rpn_bbox, 0, (size_t)batch * count * 4 * sizeof(float), s);
    if (e != hipSuccess) return mrcnn::fail(MRCNN_ERR_LAUNCH, "rpn_deltas: hipMemsetAsync: %s", hipGetErrorString(e));
    DeltaParams p;
    p.anchors = anchors; p.boxes = gt_boxes; p.gt_off = gt_off; p.match = match; p.argmax = iou_argmax;
    p.counts = static_cast<const int32_t*>(workspace);
    p.bbox = rpn_bbox; p.num_pos = num_pos;
    p.a = num_anchors; p.m = num_rows; p.count = count; p.chunks = delta_chunks(num_anchors);
    for (int i = 0; i < 4; ++i) p.std_dev[i] = std_dev[i];
    const dim3 grid((unsigned)p.chunks, (unsigned)batch);
    hipLaunchKernelGGL(positive_count_kernel, grid, dim3(kBlock), 0, s, match, num_anchors, p.chunks, static_cast<int32_t*>(workspace));
    hipLaunchKernelGGL(rpn_deltas_kernel, grid, dim3(kBlock), 0, s, p);
    return mrcnn::check_launch("rpn_deltas");
}
