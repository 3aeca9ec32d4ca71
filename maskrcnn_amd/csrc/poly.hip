// COCO polygon ground truth to run lengths on the GPU (gfx950): rleFrPoly (and with it rleFrBbox) and rleMerge of
// cocoapi/common/maskApi.c:162-202, :49-70 — what COCO.annToRLE does per annotation in serial C — for every part and every
// annotation of a data set in one call each. No host synchronisation, the same bits from run to run. The workgroup scans and
// the bitonic sort are csrc/workgroup.hpp's.
//
// mrcnn_rle_from_poly_f64, one workgroup per polygon part:
//   1 vertices -> the 5x grid ((int)(5*x + .5)), per-edge boundary-point counts max(|dX|, |dY|) + 1, scanned by the workgroup
//   2 a thread per boundary point p finds its edge in the scanned counts by binary search and computes the point AND its
//     predecessor from the edge's two vertices (no serial walk); a pair with u[p] != u[p-1] is a column crossing, kept when it
//     falls on a pixel column of the image: key = x*h + y
//   3 the reference appends h*w, sorts, differences and merges zero differences away. That loop is a PARITY rule: the run
//     boundaries are exactly the distinct keys below h*w that occur an odd number of times. So: keys are appended to LDS in
//     any order (an LDS atomic gives the slot; the sort makes the result independent of it), bitonic-sorted, every last key of
//     an equal run with an odd length is flagged, the flags are scanned, and the runs are the differences of the flagged keys.
//   A part with at most kOnChipKeys keys is one sort. A part with more is cut into RANGES of the key space, each holding at
//   most kOnChipKeys keys (found by counting; a range of one key value needs no sort, only the parity of its count): the
//   ranges are sorted one after the other and the run index and the last boundary carry over. Such a part is swept twice,
//   once to count its runs and once to write them, because a row with more runs than `capacity` is not written at all.
//   A zero-length edge (a repeated vertex) has slope 0/0 in the reference and (int)NaN as its point's minor coordinate, a value
//   that never reaches the output there (the point's u equals both neighbours'); here that point takes the vertex itself.
//
// mrcnn_rle_merge, one workgroup per group, no serial walk either: every toggle position of every row is an event; the
//   coverage (rows that are on) just before and just after it comes from binary searches in the rows' run ends; the event is
//   a boundary of the result when the predicate (coverage > 0, or == n) changes there and no earlier row of the group toggles
//   at the same position. A boundary's index in the output is the number of boundaries before it, summed over the rows from
//   per-row scans of the flags.
//
// Built with -ffp-contract=off: 5*x + .5 and ys + s*t + .5 are separately rounded in the reference (plain -O2 x86-64 C), and a
// fused multiply-add moves boundary points across pixel centres (tests/golden/poly.npz flags cases on which it does).
#include "common.hpp"
#include "workgroup.hpp"

#include <climits>

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / mrcnn::kWave;
constexpr int kOnChipKeys = 8192;        // keys one sort holds in LDS
constexpr int kCachedVerts = 2048;       // parts up to this many vertices keep grid vertices and scanned counts in LDS
constexpr int kMaxDim = 16384;
constexpr int kMaxPartPoints = 1 << 24;  // boundary points of one part
constexpr int kMaxParts = 1 << 22;
constexpr int kMaxVerts = 1 << 28;
constexpr size_t kAlign = 256;
size_t aligned(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

using mrcnn::wave_inclusive_scan;

// ------------------------------------------------------------------------------------------------ rleFrPoly
struct PolyParams {
    const double* xy;
    const int32_t* vert_off;
    const int32_t* heights;
    const int32_t* widths;
    int32_t n, total_vertices, capacity;
    int32_t* num_runs;
    uint32_t* counts;
    int32_t* num_keys;
    int32_t* edge_ws;   // [total_vertices + n]: scanned edge counts of the parts too long for LDS
};

// x[j] = (int)(scale*xy + .5); valid when the value before the cast lies inside int's range (the cast truncates toward zero)
__device__ __forceinline__ bool to_grid(double c, int& g) {
    const double t = 5.0 * c + .5;
    const bool ok = t > -2147483649.0 && t < 2147483648.0;   // false for NaN
    g = ok ? (int)t : 0;
    return ok;
}

struct Part {
    const double* xy;   // this part's vertices
    const int* eo;      // [k+1] exclusive scan of the per-edge point counts (LDS or workspace)
    const int* vx;      // [k] grid vertices in LDS, or nullptr: recomputed from xy
    const int* vy;
    int k, h, w, points;
};

__device__ __forceinline__ void vertex(const Part& a, int j, int& x, int& y) {
    if (j == a.k) j = 0;   // x[k] = x[0]
    if (a.vx) {
        x = a.vx[j];
        y = a.vy[j];
    } else {
        to_grid(a.xy[2 * (int64_t)j], x);
        to_grid(a.xy[2 * (int64_t)j + 1], y);
    }
}

// Boundary point p of the concatenated list: (u, v) as the reference's loop over edge j, step d, computes it.
__device__ __forceinline__ void boundary_point(const Part& a, int p, int& u, int& v) {
    int lo = 0, hi = a.k;   // eo[lo] <= p < eo[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.eo[mid] <= p) lo = mid; else hi = mid;
    }
    const int d = p - a.eo[lo];
    int xs, ys, xe, ye;
    vertex(a, lo, xs, ys);
    vertex(a, lo + 1, xe, ye);
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) {
        int t = xs; xs = xe; xe = t;
        t = ys; ys = ye; ye = t;
    }
    if (dx >= dy) {
        const int t = flip ? dx - d : d;
        u = t + xs;
        if (dx == 0) {
            v = ys;   // a repeated vertex: the reference's 0/0 slope; the value is never used (header comment)
        } else {
            const double s = (double)(ye - ys) / dx;
            v = (int)(ys + s * t + .5);
        }
    } else {
        const double s = (double)(xe - xs) / dy;
        const int t = flip ? dy - d : d;
        v = t + ys;
        u = (int)(xs + s * t + .5);
    }
}

// The pair (p-1, p), p >= 1: true and the key x*h + y when it is a column crossing on a pixel column of the image.
__device__ __forceinline__ bool crossing(const Part& a, int p, uint32_t& key) {
    int u, v, up, vp;
    boundary_point(a, p, u, v);
    boundary_point(a, p - 1, up, vp);
    if (u == up) return false;
    double xd = (double)(u < up ? u : u - 1);
    xd = (xd + .5) / 5.0 - .5;
    if (floor(xd) != xd || xd < 0 || xd > (double)(a.w - 1)) return false;
    double yd = (double)(v < vp ? v : vp);
    yd = (yd + .5) / 5.0 - .5;
    if (yd < 0) yd = 0; else if (yd > (double)a.h) yd = (double)a.h;
    yd = ceil(yd);
    key = (uint32_t)((int)xd * a.h + (int)yd);
    return true;
}

struct PolyShared {
    uint32_t keys[kOnChipKeys];
    int eo[kCachedVerts + 1];
    int vx[kCachedVerts];
    int vy[kCachedVerts];
    int cnt[kBlock];          // flagged keys per thread
    uint32_t lastv[kBlock];   // a thread's last flagged key
    int red[kWaves];
    long long redll[kWaves];
    int count, bad;
    uint32_t prev;
};

// Kept crossings with lo <= key < hi; `all` = every kept crossing of the part (the alias key h*w included).
__device__ int count_range(const Part& a, uint32_t lo, uint32_t hi, PolyShared& sh, int* all) {
    int in = 0, any = 0;
    for (int p = 1 + (int)threadIdx.x; p < a.points; p += kBlock) {
        uint32_t key;
        if (crossing(a, p, key)) {
            ++any;
            in += key >= lo && key < hi;
        }
    }
    in = mrcnn::block_sum<kBlock>(in, sh.red);
    if (all) *all = mrcnn::block_sum<kBlock>(any, sh.red);
    return in;
}

enum { kCountOnly = 0, kWrite = 1, kWriteIfFits = 2 };

// The m keys of [lo, hi) (m <= kOnChipKeys): emit (unless sh.keys holds them already), sort, flag by parity, and append the
// boundaries as runs nb.. of `row` (run r = boundary r - boundary r-1, `prev` = the last boundary so far, 0 at the start).
// Returns the boundaries found.
__device__ int sort_range(const Part& a, uint32_t lo, uint32_t hi, int m, PolyShared& sh, int mode, int capacity, uint32_t* row,
                          int nb, uint32_t& prev, bool emitted = false) {
    const int tid = threadIdx.x;
    if (!emitted) {
        if (tid == 0) sh.count = 0;
        __syncthreads();
        for (int p = 1 + tid; p < a.points; p += kBlock) {
            uint32_t key;
            if (crossing(a, p, key) && key >= lo && key < hi) {
                const int slot = atomicAdd(&sh.count, 1);   // any order: the sort follows
                if (slot < kOnChipKeys) sh.keys[slot] = key;
            }
        }
    }
    int n2 = 1;
    while (n2 < m) n2 <<= 1;
    __syncthreads();   // not for the padding (its slots are nobody's): the waves enter the sort together, measured 2 % faster with it
    for (int e = m + tid; e < n2; e += kBlock) sh.keys[e] = 0xffffffffu;   // slots m.. : no key was emitted there
    mrcnn::bitonic_sort<kBlock, false>(sh.keys, n2);
    // a thread owns `chunk` (<= 32) consecutive sorted keys; bit b of mask: key e0 + b ends an equal run of odd length
    const int chunk = (m + kBlock - 1) / kBlock;
    const int e0 = min(tid * chunk, m), e1 = min(e0 + chunk, m);
    uint32_t mask = 0, last = 0;
    for (int e = e0; e < e1; ++e) {
        const uint32_t val = sh.keys[e];
        if (e + 1 < m && sh.keys[e + 1] == val) continue;
        int first = 0, hi_i = e;   // lower bound of val in keys[0, e]
        while (first < hi_i) {
            const int mid = (first + hi_i) >> 1;
            if (sh.keys[mid] < val) first = mid + 1; else hi_i = mid;
        }
        if ((e - first + 1) & 1) {
            mask |= 1u << (e - e0);
            last = val;
        }
    }
    const int mine = __popc(mask);
    sh.cnt[tid] = mine;
    sh.lastv[tid] = last;
    int total;
    const int before = mrcnn::block_inclusive_scan<kBlock>(mine, sh.red, total) - mine;   // its barriers publish cnt / lastv too
    const bool write = mode == kWrite || (mode == kWriteIfFits && nb + total + 1 <= capacity);
    if (write && mine) {
        uint32_t pv = prev;
        for (int t = tid - 1; t >= 0; --t) {
            if (sh.cnt[t]) {
                pv = sh.lastv[t];
                break;
            }
        }
        int r = nb + before;
        for (int e = e0; e < e1; ++e) {
            if ((mask >> (e - e0)) & 1u) {
                const uint32_t val = sh.keys[e];
                row[r++] = val - pv;
                pv = val;
            }
        }
    }
    if (mine && before + mine == total) sh.prev = last;   // the one thread that holds the last boundary
    __syncthreads();
    if (total) prev = sh.prev;
    __syncthreads();   // sh.prev, cnt, lastv and keys are free again
    return total;
}

// Every range of a part with more than kOnChipKeys keys, in order. Returns the boundaries; writes them when `write`.
__device__ int sweep_ranges(const Part& a, int in_range, PolyShared& sh, bool write, uint32_t* row, uint32_t& prev) {
    const uint32_t area = (uint32_t)(a.h * a.w);
    uint32_t lo = 0;
    int nb = 0, rem = in_range;
    prev = 0;
    while (lo < area && rem > 0) {
        uint32_t hi = area;
        if (rem > kOnChipKeys) {   // guess: the remaining keys spread evenly
            const uint64_t span = (uint64_t)(area - lo) * (uint64_t)(kOnChipKeys * 3 / 4) / (uint64_t)rem;
            hi = lo + (uint32_t)(span > 0 ? span : 1);
        }
        int c = count_range(a, lo, hi, sh, nullptr);
        while (c > kOnChipKeys && hi - lo > 1) {
            const uint64_t span = (uint64_t)(hi - lo) * (uint64_t)(kOnChipKeys / 2) / (uint64_t)c;
            hi = lo + (uint32_t)(span > 0 ? span : 1);
            c = count_range(a, lo, hi, sh, nullptr);
        }
        if (c > kOnChipKeys) {   // one key value, more often than a sort holds: only the parity of its count matters
            if (c & 1) {
                if (write && threadIdx.x == 0) row[nb] = lo - prev;
                prev = lo;
                ++nb;
            }
        } else if (c > 0) {
            nb += sort_range(a, lo, hi, c, sh, write ? kWrite : kCountOnly, 0, row, nb, prev);
        }
        rem -= c;
        lo = hi;
    }
    return nb;
}

__global__ __launch_bounds__(kBlock) void rle_from_poly_kernel(const PolyParams p) {
    __shared__ PolyShared sh;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int v0 = p.vert_off[i], v1 = p.vert_off[i + 1], h = p.heights[i], w = p.widths[i];
    auto refuse = [&]() {
        if (tid == 0) {
            p.num_runs[i] = -1;
            p.num_keys[i] = -1;
        }
    };
    if (h < 1 || h > kMaxDim || w < 1 || w > kMaxDim || v0 < 0 || v1 <= v0 || v1 > p.total_vertices) {   // the whole workgroup
        refuse();
        return;
    }
    Part a;
    a.k = v1 - v0;
    a.h = h;
    a.w = w;
    a.xy = p.xy + 2 * (int64_t)v0;
    const bool cached = a.k <= kCachedVerts;
    int* eo = cached ? sh.eo : p.edge_ws + (int64_t)v0 + i;
    a.eo = eo;
    a.vx = cached ? sh.vx : nullptr;
    a.vy = cached ? sh.vy : nullptr;
    if (tid == 0) {
        sh.bad = 0;
        sh.count = 0;
    }
    __syncthreads();
    bool bad = false;
    for (int j = tid; j < a.k; j += kBlock) {
        int x, y;
        const bool okx = to_grid(a.xy[2 * (int64_t)j], x), oky = to_grid(a.xy[2 * (int64_t)j + 1], y);
        bad |= !okx || !oky;
        if (cached) {
            sh.vx[j] = x;
            sh.vy[j] = y;
        }
    }
    if (bad) atomicOr(&sh.bad, 1);
    __syncthreads();
    if (sh.bad) {
        refuse();
        return;
    }
    // per-edge point counts, scanned; the running total saturates just past the limit
    long long carry = 0;
    for (int base = 0; base < a.k; base += kBlock) {
        const int j = base + tid;
        long long c = 0;
        if (j < a.k) {
            int xs, ys, xe, ye;
            vertex(a, j, xs, ys);
            vertex(a, j + 1, xe, ye);
            const long long dx = llabs((long long)xe - xs), dy = llabs((long long)ye - ys);
            c = (dx > dy ? dx : dy) + 1;
        }
        long long total;
        const long long incl = mrcnn::block_inclusive_scan<kBlock>(c, sh.redll, total);
        if (j < a.k) eo[j] = (int)min(carry + incl - c, (long long)kMaxPartPoints + 1);
        carry = min(carry + total, (long long)kMaxPartPoints + 1);
    }
    if (tid == 0) eo[a.k] = (int)carry;
    __syncthreads();
    if (carry > kMaxPartPoints) {
        refuse();
        return;
    }
    a.points = (int)carry;

    const uint32_t area = (uint32_t)(h * w);
    uint32_t* row = p.counts + (int64_t)i * p.capacity;
    // one pass counts every kept crossing and keeps the keys below h*w while they fit: the ordinary part needs no second one
    int any = 0;
    for (int q = 1 + tid; q < a.points; q += kBlock) {
        uint32_t key;
        if (crossing(a, q, key)) {
            ++any;
            if (key < area) {
                const int slot = atomicAdd(&sh.count, 1);   // any order: the sort follows
                if (slot < kOnChipKeys) sh.keys[slot] = key;
            }
        }
    }
    const int all = mrcnn::block_sum<kBlock>(any, sh.red);   // its barriers publish sh.count and sh.keys
    const int in_range = sh.count;
    __syncthreads();   // everyone has read sh.count before a sweep resets it
    uint32_t prev = 0;
    int nb;
    bool written;
    if (in_range <= kOnChipKeys) {
        nb = in_range ? sort_range(a, 0, area, in_range, sh, kWriteIfFits, p.capacity, row, 0, prev, true) : 0;
        written = nb + 1 <= p.capacity;
    } else {
        nb = sweep_ranges(a, in_range, sh, false, row, prev);
        written = nb + 1 <= p.capacity;
        if (written) sweep_ranges(a, in_range, sh, true, row, prev);
    }
    if (tid == 0) {
        p.num_runs[i] = nb + 1;
        p.num_keys[i] = all;
        if (written) row[nb] = area - prev;   // the last run always ends at h*w
    }
}

// ------------------------------------------------------------------------------------------------ rleMerge
struct MergeParams {
    const int32_t* num_runs;
    const uint32_t* counts;
    int32_t n_rows, capacity;
    const int32_t* group_off;
    int32_t groups, intersect, out_capacity;
    int32_t* out_num_runs;
    uint32_t* out_counts;
    uint32_t* ends;   // [n_rows][capacity] workspace: position after run j
    int32_t* pre;     // [n_rows][capacity] workspace: boundaries among toggles 0..j of the row
};

__device__ __forceinline__ int lower_bound(const uint32_t* e, int n, uint32_t x) {   // entries < x
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int upper_bound(const uint32_t* e, int n, uint32_t x) {   // entries <= x
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void rle_merge_kernel(const MergeParams p) {
    __shared__ int s_bad, s_nb;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & (mrcnn::kWave - 1), wave = tid / mrcnn::kWave;
    const int g0 = p.group_off[g], g1 = p.group_off[g + 1];
    if (g0 < 0 || g1 < g0 || g1 > p.n_rows) {   // the whole workgroup
        if (tid == 0) p.out_num_runs[g] = -1;
        return;
    }
    const int n = g1 - g0;
    if (n == 0) {
        if (tid == 0) p.out_num_runs[g] = 0;
        return;
    }
    if (tid == 0) {
        s_bad = 0;
        s_nb = 0;
    }
    __syncthreads();
    for (int q = tid; q < n; q += kBlock) {
        const int nr = p.num_runs[g0 + q];
        if (nr < 0 || nr > p.capacity) atomicOr(&s_bad, 1);
    }
    __syncthreads();
    if (s_bad) {   // a row whose counts were never written
        if (tid == 0) p.out_num_runs[g] = -1;
        return;
    }
    uint32_t* out = p.out_counts + (int64_t)g * p.out_capacity;
    if (n == 1) {   // rleMerge's n == 1: a copy
        const int nr = p.num_runs[g0];
        if (tid == 0) p.out_num_runs[g] = nr;
        if (nr <= p.out_capacity)
            for (int j = tid; j < nr; j += kBlock) out[j] = p.counts[(int64_t)g0 * p.capacity + j];
        return;
    }
    // run ends, a wave per row
    for (int q = wave; q < n; q += kWaves) {
        const int64_t row = (int64_t)(g0 + q) * p.capacity;
        const int nr = p.num_runs[g0 + q];
        uint32_t end = 0;
        for (int base = 0; base < nr; base += mrcnn::kWave) {
            const int j = base + lane;
            const uint32_t e = end + wave_inclusive_scan(j < nr ? p.counts[row + j] : 0u, lane);
            if (j < nr) p.ends[row + j] = e;
            end = __shfl(e, mrcnn::kWave - 1);
        }
    }
    __syncthreads();
    // every toggle (the end of a run that is not the row's last): is it a boundary of the result?
    for (int q = 0; q < n; ++q) {
        const int64_t row = (int64_t)(g0 + q) * p.capacity;
        const int nr = p.num_runs[g0 + q];
        for (int j = tid; j < nr - 1; j += kBlock) {
            const uint32_t pos = p.ends[row + j];
            int before = 0, after = 0;
            bool earlier = false;
            for (int r = 0; r < n; ++r) {
                const uint32_t* e = p.ends + (int64_t)(g0 + r) * p.capacity;
                const int nrr = p.num_runs[g0 + r];
                const int lb = lower_bound(e, nrr, pos), ub = upper_bound(e, nrr, pos);
                // pixel x lies in run (number of ends <= x); odd runs are on
                before += pos > 0 && (lb & 1) && lb < nrr;
                after += (ub & 1) && ub < nrr;
                earlier |= r < q && ub > lb && lb < nrr - 1;
            }
            const bool pb = p.intersect ? before == n : before > 0, pa = p.intersect ? after == n : after > 0;
            p.pre[row + j] = (!earlier && pb != pa) ? 1 : 0;
        }
    }
    __syncthreads();
    for (int q = wave; q < n; q += kWaves) {
        const int64_t row = (int64_t)(g0 + q) * p.capacity;
        const int nt = p.num_runs[g0 + q] - 1;
        int sum = 0;
        for (int base = 0; base < nt; base += mrcnn::kWave) {
            const int j = base + lane;
            const int s = sum + wave_inclusive_scan(j < nt ? p.pre[row + j] : 0, lane);
            if (j < nt) p.pre[row + j] = s;
            sum = __shfl(s, mrcnn::kWave - 1);
        }
        if (lane == 0 && sum) atomicAdd(&s_nb, sum);   // an integer sum: the same in any order
    }
    __syncthreads();
    const int nb = s_nb;
    if (tid == 0) p.out_num_runs[g] = nb + 1;
    if (nb + 1 > p.out_capacity) return;   // the whole workgroup: the row is not written
    // positions of the boundaries, each at its rank; the closing position is the pixel count
    for (int q = 0; q < n; ++q) {
        const int64_t row = (int64_t)(g0 + q) * p.capacity;
        const int nr = p.num_runs[g0 + q];
        for (int j = tid; j < nr - 1; j += kBlock) {
            if (p.pre[row + j] - (j ? p.pre[row + j - 1] : 0) == 0) continue;
            const uint32_t pos = p.ends[row + j];
            int rank = 0;
            for (int r = 0; r < n; ++r) {
                const int64_t rr = (int64_t)(g0 + r) * p.capacity;
                const int lt = lower_bound(p.ends + rr, p.num_runs[g0 + r] - 1, pos);   // toggles before pos
                if (lt > 0) rank += p.pre[rr + lt - 1];
            }
            out[rank] = pos;
        }
    }
    if (tid == 0) {
        const int nr0 = p.num_runs[g0];
        out[nb] = nr0 > 0 ? p.ends[(int64_t)g0 * p.capacity + nr0 - 1] : 0u;
    }
    __syncthreads();
    // positions -> run lengths in place, from the last chunk down: a chunk reads nothing a later chunk has rewritten
    for (int c = nb / kBlock; c >= 0; --c) {
        const int r = c * kBlock + tid;
        uint32_t cur = 0, pv = 0;
        if (r <= nb) {
            cur = out[r];
            pv = r ? out[r - 1] : 0u;
        }
        __syncthreads();
        if (r <= nb) out[r] = cur - pv;
    }
}

}  // namespace

extern "C" int32_t mrcnn_rle_from_poly_onchip_keys(void) { return kOnChipKeys; }

extern "C" size_t mrcnn_rle_from_poly_workspace_bytes(int32_t n, int32_t total_vertices) {
    if (n <= 0 || n > kMaxParts || total_vertices < 0 || total_vertices > kMaxVerts) return 0;
    return aligned(((size_t)total_vertices + (size_t)n) * sizeof(int32_t));
}

extern "C" int mrcnn_rle_from_poly_f64(const double* xy, int32_t total_vertices, const int32_t* vert_off, const int32_t* heights,
                                       const int32_t* widths, int32_t n, int32_t capacity, int32_t* num_runs, uint32_t* counts,
                                       int32_t* num_keys, void* workspace, size_t workspace_bytes, mrcnn_stream_t stream) {
    MRCNN_REQUIRE(n >= 0 && n <= kMaxParts, "rle_from_poly: n=%d must be in [0, %d]", n, kMaxParts);
    MRCNN_REQUIRE(total_vertices >= 0 && total_vertices <= kMaxVerts, "rle_from_poly: %d vertices, at most %d in one call",
                  total_vertices, kMaxVerts);
    MRCNN_REQUIRE(capacity >= 1, "rle_from_poly: capacity=%d must be >= 1", capacity);
    if (n == 0) return MRCNN_OK;
    MRCNN_REQUIRE(vert_off && heights && widths && num_runs && counts && num_keys && (xy || total_vertices == 0),
                  "rle_from_poly: null pointer");
    const size_t need = mrcnn_rle_from_poly_workspace_bytes(n, total_vertices);
    MRCNN_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                  "rle_from_poly: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, workspace_bytes);
    PolyParams p;
    p.xy = xy; p.vert_off = vert_off; p.heights = heights; p.widths = widths;
    p.n = n; p.total_vertices = total_vertices; p.capacity = capacity;
    p.num_runs = num_runs; p.counts = counts; p.num_keys = num_keys;
    p.edge_ws = static_cast<int32_t*>(workspace);
    hipLaunchKernelGGL(rle_from_poly_kernel, dim3((unsigned)n), dim3(kBlock), 0, mrcnn::as_stream(stream), p);
    return mrcnn::check_launch("rle_from_poly");
}

extern "C" size_t mrcnn_rle_merge_workspace_bytes(int32_t n_rows, int32_t capacity) {
    if (n_rows <= 0 || capacity <= 0) return 0;
    return 2 * aligned((size_t)n_rows * (size_t)capacity * 4);
}

extern "C" int mrcnn_rle_merge(const int32_t* num_runs, const uint32_t* counts, int32_t n_rows, int32_t capacity,
                               const int32_t* group_off, int32_t groups, int32_t intersect, int32_t out_capacity,
                               int32_t* out_num_runs, uint32_t* out_counts, void* workspace, size_t workspace_bytes,
                               mrcnn_stream_t stream) {
    MRCNN_REQUIRE(n_rows >= 0 && capacity >= 1 && out_capacity >= 1, "rle_merge: n_rows=%d (>= 0), capacities %d, %d (>= 1)",
                  n_rows, capacity, out_capacity);
    MRCNN_REQUIRE(groups >= 0 && (intersect == 0 || intersect == 1), "rle_merge: groups=%d (>= 0), intersect=%d (0 or 1)", groups,
                  intersect);
    if (groups == 0) return MRCNN_OK;
    MRCNN_REQUIRE(group_off && out_num_runs && out_counts && (n_rows == 0 || (num_runs && counts)), "rle_merge: null pointer");
    const size_t need = mrcnn_rle_merge_workspace_bytes(n_rows, capacity);
    MRCNN_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0),
                  "rle_merge: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, workspace_bytes);
    MergeParams p;
    p.num_runs = num_runs; p.counts = counts; p.n_rows = n_rows; p.capacity = capacity;
    p.group_off = group_off; p.groups = groups; p.intersect = intersect; p.out_capacity = out_capacity;
    p.out_num_runs = out_num_runs; p.out_counts = out_counts;
    p.ends = static_cast<uint32_t*>(workspace);
    p.pre = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + aligned((size_t)n_rows * (size_t)capacity * 4));
    hipLaunchKernelGGL(rle_merge_kernel, dim3((unsigned)groups), dim3(kBlock), 0, mrcnn::as_stream(stream), p);
    return mrcnn::check_launch("rle_merge");
}
