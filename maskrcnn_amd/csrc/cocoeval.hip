// COCO evaluation on the GPU (gfx950): the per-pair and per-group work of COCOeval.evaluate() —
//   mrcnn_rle_iou_f64   rleIou  of cocoapi/common/maskApi.c:77-96 on two run-list tables (the layout mrcnn_rle_encode_u8 writes)
//   mrcnn_bbox_iou_f64  bbIou   of maskApi.c:109-120 on (x, y, w, h) float64 boxes
//   mrcnn_coco_match    the matching loop of evaluateImg, pycocotools/cocoeval.py:251-300
// all GROUPED: one call serves K (image, category) groups whose members are named by device offset arrays, so an
// evaluation of thousands of groups of a few masks each is one launch group. No atomics, no host synchronisation.
//
// rleIou is not ported as its serial two-pointer merge. Intersection and union are integer sums, exact in any order:
//   1 rle_ends_kernel  a wave per mask: inclusive scan of the counts -> run end positions, and the on pixels up to each run
//   2 rle_iou_kernel   a wave per (detection, ground truth) pair: the detection's on runs are spread over the lanes; a run
//                      [s, e) overlaps the ground truth in F(e) - F(s) pixels, F(x) = on pixels of the ground truth before
//                      position x, found by binary search in its end positions. union = area_d + area_g - intersection.
// The wave scan and the wave reduction are csrc/workgroup.hpp's.
// The reference's bounding-box pre-test (rleIou calls bbIou on rleToBbox first and keeps its 0) changes no bit: boxes that
// do not overlap hold masks that do not overlap, and an empty intersection is (double)0 / (double)1 = +0.0 too.
//
// Built with -ffp-contract=off: bbIou's da+ga-i with i=w*h must stay separately rounded (the reference codec is plain -O2
// x86-64 C: no FMA).
#include "common.hpp"
#include "workgroup.hpp"

#include <climits>

namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / mrcnn::kWave;
constexpr size_t kAlign = 256;
size_t aligned(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

// ------------------------------------------------------------------------------------------------ group lookup
// Element e of the output belongs to the last group k with out_off[k] <= e (empty groups share their start with the next
// one and are never chosen). Returns false for an element outside every group's matrix.
struct Groups {
    const int32_t* dt_off;
    const int32_t* gt_off;
    const int64_t* out_off;
    int32_t groups, n_dt, n_gt;
};

struct Pair {
    int32_t di, gi;   // rows of the detection and ground-truth tables
    int32_t g_local;  // ground truth within its group (for nothing but clarity)
};

__device__ __forceinline__ bool find_pair(const Groups& q, int64_t e, Pair& r) {
    int lo = 0, hi = q.groups;   // invariant: out_off[lo] <= e (checked below), answer in [lo, hi)
    if (q.out_off[0] > e) return false;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (q.out_off[mid] <= e) lo = mid; else hi = mid;
    }
    const int k = lo;
    const int64_t local = e - q.out_off[k];
    const int32_t d0 = q.dt_off[k], g0 = q.gt_off[k];
    const int64_t m = (int64_t)q.dt_off[k + 1] - d0, n = (int64_t)q.gt_off[k + 1] - g0;
    if (m <= 0 || n <= 0 || local >= m * n || e >= q.out_off[k + 1]) return false;
    const int64_t g = local / m, d = local - g * m;   // maskApi's o[g*m + d]
    r.di = d0 + (int32_t)d;
    r.gi = g0 + (int32_t)g;
    r.g_local = (int32_t)g;
    return d0 >= 0 && g0 >= 0 && r.di < q.n_dt && r.gi < q.n_gt;   // offsets that point outside the tables read nothing
}

// ------------------------------------------------------------------------------------------------ rleIou
struct Table {
    const int32_t* num_runs;
    const uint32_t* counts;
    int32_t n, capacity;
    uint32_t* ends;     // [n][capacity] workspace: position after run j
    uint32_t* on_upto;  // [n][capacity] workspace: on pixels in runs 0..j
    uint32_t* area;     // [n] workspace
};

__global__ __launch_bounds__(kBlock) void rle_ends_kernel(const Table a, const Table b) {
    const int lane = threadIdx.x & (mrcnn::kWave - 1);
    int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / mrcnn::kWave;
    const Table& t = w < a.n ? a : b;
    if (w >= a.n) w -= a.n;
    if (w >= t.n) return;
    const int nr = t.num_runs[w];
    if (nr > t.capacity || nr < 0) {   // the encoder wrote no counts for this mask: its pairs report -1
        if (lane == 0) t.area[w] = 0;
        return;
    }
    const int64_t row = w * (int64_t)t.capacity;
    uint32_t end = 0, on = 0;
    for (int base = 0; base < nr; base += mrcnn::kWave) {
        const int j = base + lane;
        const uint32_t c = j < nr ? t.counts[row + j] : 0u;
        const uint32_t e = end + mrcnn::wave_inclusive_scan(c, lane);
        const uint32_t o = on + mrcnn::wave_inclusive_scan((j & 1) ? c : 0u, lane);
        if (j < nr) {
            t.ends[row + j] = e;
            t.on_upto[row + j] = o;
        }
        end = __shfl(e, mrcnn::kWave - 1);
        on = __shfl(o, mrcnn::kWave - 1);
    }
    if (lane == 0) t.area[w] = on;
}

// on pixels of the mask before position x (0 <= x; x past the mask's end counts the whole mask)
__device__ __forceinline__ uint32_t on_before(const uint32_t* ends, const uint32_t* on_upto, int nr, uint32_t x) {
    int lo = 0, hi = nr;   // r = number of runs that end at or before x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ends[mid] <= x) lo = mid + 1; else hi = mid;
    }
    const int r = lo;
    if (r == 0) return 0;   // inside run 0, which is off
    uint32_t v = on_upto[r - 1];
    if ((r & 1) && r < nr) v += x - ends[r - 1];   // inside on run r
    return v;
}

struct IouParams {
    Groups q;
    Table dt, gt;
    const uint8_t* iscrowd;
    double* out;
    int64_t out_len;
};

__global__ __launch_bounds__(kBlock) void rle_iou_kernel(const IouParams p) {
    const int lane = threadIdx.x & (mrcnn::kWave - 1);
    const int64_t e = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / mrcnn::kWave;
    if (e >= p.out_len) return;
    Pair pr;
    if (!find_pair(p.q, e, pr)) return;   // the whole wave takes this branch
    const int nd = p.dt.num_runs[pr.di], ng = p.gt.num_runs[pr.gi];
    if (nd > p.dt.capacity || ng > p.gt.capacity || nd < 0 || ng < 0) {
        if (lane == 0) p.out[e] = -1.0;   // the reference's "cannot compare"
        return;
    }
    const uint32_t* de = p.dt.ends + (int64_t)pr.di * p.dt.capacity;
    const uint32_t* ge = p.gt.ends + (int64_t)pr.gi * p.gt.capacity;
    const uint32_t* go = p.gt.on_upto + (int64_t)pr.gi * p.gt.capacity;
    uint32_t inter = 0;
    for (int j = 1 + 2 * lane; j < nd; j += 2 * mrcnn::kWave) {   // on runs are the odd ones
        const uint32_t s = de[j - 1], t = de[j];
        if (t > s) inter += on_before(ge, go, ng, t) - on_before(ge, go, ng, s);
    }
    inter = mrcnn::wave_reduce(inter, [](uint32_t a, uint32_t b) { return a + b; });
    if (lane == 0) {
        const uint32_t area_d = p.dt.area[pr.di], area_g = p.gt.area[pr.gi];
        const bool crowd = p.iscrowd != nullptr && p.iscrowd[pr.gi] != 0;
        uint32_t u = area_d + area_g - inter;
        if (inter == 0) u = 1; else if (crowd) u = area_d;
        p.out[e] = (double)inter / (double)u;
    }
}

// ------------------------------------------------------------------------------------------------ bbIou
struct BoxParams {
    Groups q;
    const double* dt;
    const double* gt;
    const uint8_t* iscrowd;
    double* out;
    int64_t out_len;
};

__global__ __launch_bounds__(kBlock) void bbox_iou_kernel(const BoxParams p) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.out_len) return;
    Pair pr;
    if (!find_pair(p.q, e, pr)) return;
    const double* D = p.dt + 4 * (int64_t)pr.di;
    const double* G = p.gt + 4 * (int64_t)pr.gi;
    const bool crowd = p.iscrowd != nullptr && p.iscrowd[pr.gi] != 0;
    const double ga = G[2] * G[3], da = D[2] * D[3];
    double o = 0;
    const double w = fmin(D[2] + D[0], G[2] + G[0]) - fmax(D[0], G[0]);
    if (!(w <= 0)) {
        const double h = fmin(D[3] + D[1], G[3] + G[1]) - fmax(D[1], G[1]);
        if (!(h <= 0)) {
            const double i = w * h;
            const double u = crowd ? da : da + ga - i;
            o = i / u;
        }
    }
    p.out[e] = o;
}

// ------------------------------------------------------------------------------------------------ evaluateImg
struct MatchParams {
    Groups q;
    const double* ious;
    int64_t ious_len;
    const double* dt_area;
    const double* gt_area;
    const uint8_t* gt_iscrowd;
    const double* area_ranges;   // [A][2]
    const double* thresholds;    // [T]
    int32_t num_ranges, num_thresholds;
    int32_t* dt_match;           // [A][T][N]
    int32_t* gt_match;           // [A][T][M]
    uint8_t* dt_ignore;          // [A][T][N]
    uint8_t* gt_ignore;          // [A][M]
};

// One thread per (group, area range, threshold) runs the reference's loop: it is short, and its early break depends on order.
__global__ __launch_bounds__(kBlock) void coco_match_kernel(const MatchParams p) {
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int T = p.num_thresholds, A = p.num_ranges;
    if (tid >= (int64_t)p.q.groups * A * T) return;
    const int t = (int)(tid % T);
    const int a = (int)((tid / T) % A);
    const int k = (int)(tid / ((int64_t)T * A));
    const int d0 = p.q.dt_off[k], g0 = p.q.gt_off[k];
    const int D = p.q.dt_off[k + 1] - d0, G = p.q.gt_off[k + 1] - g0;
    if (D < 0 || G < 0 || d0 < 0 || g0 < 0 || (int64_t)d0 + D > p.q.n_dt || (int64_t)g0 + G > p.q.n_gt) return;
    const double lo = p.area_ranges[2 * a], hi = p.area_ranges[2 * a + 1];
    const int64_t at = (int64_t)a * T + t;
    int32_t* dtm = p.dt_match + at * p.q.n_dt + d0;
    uint8_t* dtig = p.dt_ignore + at * p.q.n_dt + d0;
    int32_t* gtm = p.gt_match + at * p.q.n_gt + g0;
    const double* garea = p.gt_area + g0;
    const uint8_t* crowd = p.gt_iscrowd + g0;
    // g['_ignore'] = g['ignore'] or area < aRng[0] or area > aRng[1], with ignore = iscrowd (cocoeval.py:109-110, :251-255)
    auto ignored = [&](int g) { return crowd[g] != 0 || garea[g] < lo || garea[g] > hi; };
    for (int g = 0; g < G; ++g) gtm[g] = 0;
    if (t == 0)
        for (int g = 0; g < G; ++g) p.gt_ignore[(int64_t)a * p.q.n_gt + g0 + g] = ignored(g) ? 1 : 0;

    const int64_t base = p.q.out_off[k];
    const bool have_ious = D > 0 && G > 0 && base >= 0 && base + (int64_t)D * G <= p.ious_len;
    const double thr = p.thresholds[t];
    for (int d = 0; d < D; ++d) {
        int m = -1;
        bool m_ignored = false;
        if (have_ious) {
            double iou = fmin(thr, 1 - 1e-10);
            // the stable argsort of _ignore (:258): the regular ground truths in input order, then the ignored ones
            for (int pass = 0; pass < 2; ++pass) {
                // "if dt matched to reg gt, and on ignore gt, stop" (:284): a match from pass 0 is a regular one
                if (pass == 1 && m > -1) break;
                for (int g = 0; g < G; ++g) {
                    if (ignored(g) != (pass == 1)) continue;
                    if (gtm[g] > 0 && !crowd[g]) continue;
                    const double v = p.ious[base + (int64_t)g * D + d];
                    if (v < iou) continue;
                    iou = v;
                    m = g;
                    m_ignored = pass == 1;
                }
            }
        }
        uint8_t ig = 0;
        if (m > -1) {
            ig = m_ignored ? 1 : 0;
            gtm[m] = d + 1;
        } else {
            const double ar = p.dt_area[d0 + d];
            ig = (ar < lo || ar > hi) ? 1 : 0;   // unmatched detections outside the area range are ignored (:299-300)
        }
        dtm[d] = m + 1;
        dtig[d] = ig;
    }
}

bool groups_ok(int32_t groups) { return groups >= 0; }

}  // namespace

extern "C" size_t mrcnn_rle_iou_workspace_bytes(int32_t n_dt, int32_t dt_capacity, int32_t n_gt, int32_t gt_capacity) {
    if (n_dt < 0 || n_gt < 0 || dt_capacity < 0 || gt_capacity < 0) return 0;
    const size_t d = (size_t)n_dt * (size_t)dt_capacity, g = (size_t)n_gt * (size_t)gt_capacity;
    return 2 * aligned(d * 4) + 2 * aligned(g * 4) + aligned((size_t)n_dt * 4) + aligned((size_t)n_gt * 4);
}

extern "C" int mrcnn_rle_iou_f64(const int32_t* dt_num_runs, const uint32_t* dt_counts, int32_t n_dt, int32_t dt_capacity,
                                 const int32_t* gt_num_runs, const uint32_t* gt_counts, int32_t n_gt, int32_t gt_capacity,
                                 const uint8_t* iscrowd, const int32_t* dt_off, const int32_t* gt_off, const int64_t* out_off,
                                 int32_t groups, double* out, int64_t out_len, void* workspace, size_t workspace_bytes,
                                 mrcnn_stream_t stream) {
    MRCNN_REQUIRE(n_dt >= 0 && n_gt >= 0 && dt_capacity >= 1 && gt_capacity >= 1,
                  "rle_iou: n_dt=%d n_gt=%d (>= 0), capacities %d, %d (>= 1)", n_dt, n_gt, dt_capacity, gt_capacity);
    MRCNN_REQUIRE(groups_ok(groups) && out_len >= 0 && out_len <= (int64_t)INT_MAX * kWavesPerBlock,
                  "rle_iou: groups=%d, out_len=%lld out of range", groups, (long long)out_len);
    if (groups == 0 || out_len == 0 || n_dt == 0 || n_gt == 0) return MRCNN_OK;
    MRCNN_REQUIRE(dt_num_runs && dt_counts && gt_num_runs && gt_counts && dt_off && gt_off && out_off && out,
                  "rle_iou: null pointer");
    const size_t need = mrcnn_rle_iou_workspace_bytes(n_dt, dt_capacity, n_gt, gt_capacity);
    MRCNN_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                  "rle_iou: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, workspace_bytes);
    IouParams p;
    p.q = Groups{dt_off, gt_off, out_off, groups, n_dt, n_gt};
    p.dt = Table{dt_num_runs, dt_counts, n_dt, dt_capacity, nullptr, nullptr, nullptr};
    p.gt = Table{gt_num_runs, gt_counts, n_gt, gt_capacity, nullptr, nullptr, nullptr};
    const size_t d = (size_t)n_dt * (size_t)dt_capacity, g = (size_t)n_gt * (size_t)gt_capacity;
    char* ws = static_cast<char*>(workspace);
    p.dt.ends = reinterpret_cast<uint32_t*>(ws);     ws += aligned(d * 4);
    p.dt.on_upto = reinterpret_cast<uint32_t*>(ws);  ws += aligned(d * 4);
    p.gt.ends = reinterpret_cast<uint32_t*>(ws);     ws += aligned(g * 4);
    p.gt.on_upto = reinterpret_cast<uint32_t*>(ws);  ws += aligned(g * 4);
    p.dt.area = reinterpret_cast<uint32_t*>(ws);     ws += aligned((size_t)n_dt * 4);
    p.gt.area = reinterpret_cast<uint32_t*>(ws);
    p.iscrowd = iscrowd;
    p.out = out;
    p.out_len = out_len;
    hipStream_t s = mrcnn::as_stream(stream);
    const int64_t masks = (int64_t)n_dt + n_gt;
    hipLaunchKernelGGL(rle_ends_kernel, dim3((unsigned)((masks + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, s, p.dt,
                       p.gt);
    hipLaunchKernelGGL(rle_iou_kernel, dim3((unsigned)((out_len + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, s, p);
    return mrcnn::check_launch("rle_iou");
}

extern "C" int mrcnn_bbox_iou_f64(const double* dt_boxes, int32_t n_dt, const double* gt_boxes, int32_t n_gt,
                                  const uint8_t* iscrowd, const int32_t* dt_off, const int32_t* gt_off, const int64_t* out_off,
                                  int32_t groups, double* out, int64_t out_len, mrcnn_stream_t stream) {
    MRCNN_REQUIRE(n_dt >= 0 && n_gt >= 0, "bbox_iou: n_dt=%d n_gt=%d must be >= 0", n_dt, n_gt);
    MRCNN_REQUIRE(groups_ok(groups) && out_len >= 0 && out_len <= (int64_t)INT_MAX * kWavesPerBlock,
                  "bbox_iou: groups=%d, out_len=%lld out of range", groups, (long long)out_len);
    if (groups == 0 || out_len == 0 || n_dt == 0 || n_gt == 0) return MRCNN_OK;
    MRCNN_REQUIRE(dt_boxes && gt_boxes && dt_off && gt_off && out_off && out, "bbox_iou: null pointer");
    BoxParams p;
    p.q = Groups{dt_off, gt_off, out_off, groups, n_dt, n_gt};
    p.dt = dt_boxes; p.gt = gt_boxes; p.iscrowd = iscrowd; p.out = out; p.out_len = out_len;
    hipLaunchKernelGGL(bbox_iou_kernel, dim3((unsigned)((out_len + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       mrcnn::as_stream(stream), p);
    return mrcnn::check_launch("bbox_iou");
}

extern "C" int mrcnn_coco_match(const double* ious, int64_t ious_len, const int32_t* dt_off, const int32_t* gt_off,
                                const int64_t* out_off, int32_t groups, const double* dt_area, int32_t n_dt,
                                const double* gt_area, const uint8_t* gt_iscrowd, int32_t n_gt, const double* area_ranges,
                                int32_t num_ranges, const double* thresholds, int32_t num_thresholds, int32_t* dt_match,
                                int32_t* gt_match, uint8_t* dt_ignore, uint8_t* gt_ignore, mrcnn_stream_t stream) {
    MRCNN_REQUIRE(n_dt >= 0 && n_gt >= 0 && ious_len >= 0, "coco_match: n_dt=%d n_gt=%d ious_len=%lld must be >= 0", n_dt, n_gt,
                  (long long)ious_len);
    MRCNN_REQUIRE(groups_ok(groups) && num_ranges >= 1 && num_thresholds >= 1 &&
                      (int64_t)groups * num_ranges * num_thresholds <= (int64_t)INT_MAX,
                  "coco_match: groups=%d x %d area ranges x %d thresholds out of range", groups, num_ranges, num_thresholds);
    if (groups == 0) return MRCNN_OK;
    MRCNN_REQUIRE(dt_off && gt_off && out_off && area_ranges && thresholds, "coco_match: null pointer");
    MRCNN_REQUIRE(n_dt == 0 || (dt_area && dt_match && dt_ignore), "coco_match: null detection pointer");
    MRCNN_REQUIRE(n_gt == 0 || (gt_area && gt_iscrowd && gt_match && gt_ignore), "coco_match: null ground-truth pointer");
    MRCNN_REQUIRE(ious_len == 0 || ious, "coco_match: null ious");
    MatchParams p;
    p.q = Groups{dt_off, gt_off, out_off, groups, n_dt, n_gt};
    p.ious = ious; p.ious_len = ious_len; p.dt_area = dt_area; p.gt_area = gt_area; p.gt_iscrowd = gt_iscrowd;
    p.area_ranges = area_ranges; p.thresholds = thresholds; p.num_ranges = num_ranges; p.num_thresholds = num_thresholds;
    p.dt_match = dt_match; p.gt_match = gt_match; p.dt_ignore = dt_ignore; p.gt_ignore = gt_ignore;
    const int64_t threads = (int64_t)groups * num_ranges * num_thresholds;
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       mrcnn::as_stream(stream), p);
    return mrcnn::check_launch("coco_match");
}
