// Workgroup primitives shared by the non-conv kernels (gfx950, wave64): wave and workgroup scans and reductions, the chunked
// scan of a global array, the LDS bitonic sort, and rleToString's group loop. Function templates only. Every routine that
// has a barrier in it must be reached by ALL kThreads threads of the workgroup (kThreads == blockDim.x, a multiple of the
// wave), and every wave routine by all 64 lanes. The barriers are common.hpp's __syncthreads, so a -DMRCNN_SYNC_FUZZ build
// fuzzes them here as well. Each routine states its barrier contract; the callers rely on it and add no barrier of their own
// around it.
#pragma once
#include "common.hpp"

namespace mrcnn {

// ------------------------------------------------------------------------------------------------ one wave
// Inclusive prefix sum over the lanes of a wave. No LDS, no barrier.
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v, int lane) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// op over the lanes of a wave, the result in every lane. No LDS, no barrier.
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v = op(v, __shfl_xor(v, d));
    return v;
}

// ------------------------------------------------------------------------------------------------ one value per thread
// Inclusive prefix sum of one value per thread in thread order; `total` is the sum, in every thread. red: LDS [kThreads / kWave].
// Barriers: two. On entry no other thread may still be reading `red`. The first barrier also publishes whatever the caller
// wrote to LDS before the call; the second is the last thing done, so `red` may be reused at once.
template <int kThreads, class T>
__device__ __forceinline__ T block_inclusive_scan(T v, T* red, T& total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    v = wave_inclusive_scan(v, lane);
    if (lane == kWave - 1) red[wave] = v;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kThreads / kWave; ++i) {
        const T r = red[i];
        if (i < wave) before += r;
        all += r;
    }
    __syncthreads();
    total = all;
    return v + before;
}

// op over one value per thread, the result in every thread. red: LDS [kThreads / kWave]. Barriers: as block_inclusive_scan.
template <int kThreads, class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T* red, Op op) {
    v = wave_reduce(v, op);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    T r = red[0];
#pragma unroll
    for (int i = 1; i < kThreads / kWave; ++i) r = op(r, red[i]);
    __syncthreads();
    return r;
}

// Sum of one value per thread, in every thread. On the scan, not on block_reduce: in rle_from_poly_kernel, which uses both,
// the butterfly as a second code shape cost eight VGPRs. Barriers: as block_inclusive_scan.
template <int kThreads, class T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    T total;
    block_inclusive_scan<kThreads>(v, red, total);
    return total;
}

// ------------------------------------------------------------------------------------------------ a global array
// Exclusive scan of in[0, count) into out[0, count) under an associative `join(earlier, later)` by one workgroup: every thread
// folds a contiguous chunk, the chunk sums are scanned through LDS, a second walk over the chunk writes the prefixes. Returns
// the total, in every thread. out must not overlap in (out[i] is stored before in[i] is read again). lds: [2 * kThreads].
// Barriers: 1 + log2(kThreads). On entry no other thread may still be reading `lds`. There is NO barrier after the last read
// of `lds`: the caller puts one before it writes there again. Nothing of `out` is published to other threads.
template <int kThreads, class T, class Join>
__device__ T chunked_exclusive_scan(const T* in, T* out, int64_t count, T identity, T* lds, Join join) {
    const int t = threadIdx.x;
    const int64_t chunk = (count + kThreads - 1) / kThreads;
    const int64_t lo = min((int64_t)t * chunk, count), hi = min(lo + chunk, count);
    T acc = identity;
    for (int64_t i = lo; i < hi; ++i) acc = join(acc, in[i]);
    int cur = 0;
    lds[t] = acc;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        T v = lds[cur * kThreads + t];
        if (t >= d) v = join(lds[cur * kThreads + t - d], v);
        lds[(cur ^ 1) * kThreads + t] = v;
        cur ^= 1;
        __syncthreads();
    }
    T r = t > 0 ? lds[cur * kThreads + t - 1] : identity;
    for (int64_t i = lo; i < hi; ++i) {
        out[i] = r;
        r = join(r, in[i]);
    }
    return lds[cur * kThreads + kThreads - 1];   // read last: a caller that needs it in one thread only reads it there
}

// ------------------------------------------------------------------------------------------------ LDS sort
// Bitonic sort of keys[0, n) in LDS, n a power of two (the caller pads): n / 2 compare-exchanges per step, spread over the
// threads. Equal keys may end in either order.
// Barriers: one on entry and one after every step (a single one when n == 1). So the keys may be written by any thread
// right up to the call, the sorted keys are visible to every thread on return, and the caller adds no barrier on either
// side.
template <int kThreads, bool kDescending, class T>
__device__ __forceinline__ void bitonic_sort(T* keys, int n) {
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += kThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const T a = keys[i], b = keys[i + j];
                const bool first = (i & k) == 0;   // the pair lies in a run that is sorted in the requested direction
                if ((kDescending ? a < b : a > b) == first) {   // ONE compare: `first ? a > b : a < b` cost NMS 2-6 %, polygons 5 %
                    keys[i] = b;
                    keys[i + j] = a;
                }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------ rleToString
// The group loop of rleToString (cocoapi/common/maskApi.c:204-216) for one value, a long there: 5 bits a character, low
// group first. Returns the characters; writes them when kWrite and dst is not null. V is long long, or int where the caller knows the
// value fits (the encoder's |x| <= 2^28: a 64-bit loop there costs rle_emit_kernel<true> two VGPRs and a wave of occupancy).
template <bool kWrite, class V>
__device__ __forceinline__ int rle_put_value(uint8_t* dst, V x) {
    int k = 0;
    bool more;
    do {
        int c = (int)(x & 31);
        x >>= 5;   // arithmetic
        more = (c & 16) ? x != -1 : x != 0;
        if (more) c |= 32;
        if (kWrite && dst) dst[k] = (uint8_t)(c + 48);
        ++k;
    } while (more);
    return k;
}

}  // namespace mrcnn
