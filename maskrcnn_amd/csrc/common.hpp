// Shared host-side helpers for libmaskrcnn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "maskrcnn_hip.h"

namespace mrcnn {

// thread-local error message behind mrcnn_last_error()
char* error_buffer();
int fail(int code, const char* fmt, ...);

inline hipStream_t as_stream(mrcnn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Check the launch that was just issued (no synchronisation).
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MRCNN_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return MRCNN_OK;
}

constexpr int kWave = 64;  // gfx950 wavefront

// Per-device launch state. A process may drive several GPUs (one torch device guard per call); nothing below may be
// cached per process. Both helpers are keyed by hipGetDevice() of the calling thread.
//   ensure_dynamic_lds: hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel, size) — kernels that
//                       use more than 64 KB of dynamic LDS need it on EVERY device they are launched on;
//   device_cu_count:    multiProcessorCount of the current device (persistent-grid sizing), 0 on failure.
int ensure_dynamic_lds(const void* kernel, size_t lds_bytes, const char* who);
int device_cu_count();

// The launch tail every persistent launcher shares. Each launcher keeps its own grid rule (they differ for measured reasons,
// stated at each site); what they share is the device query, the XCD rounding and the grant / launch / check sequence.
//   query_cus:     the CU count of the current device, or THE answer to a failed query: MRCNN_ERR_LAUNCH,
//                  "<who>: cannot query the device";
//   whole_xcds:    CUs rounded down to whole XCDs (8 per device), so every XCD runs the same number of persistent workgroups;
//   launch_kernel: ensure_dynamic_lds, the launch through a kernel function pointer, check_launch. `who` names the entry point
//                  (error prefix of the LDS grant), `kernel_name` the kernel (error prefix of the launch check);
//   launch_one_per_cu: the three together for the grid rule min(units, whole_xcds(CUs)).
inline int query_cus(const char* who, int& cus) {
    cus = device_cu_count();
    return cus > 0 ? MRCNN_OK : fail(MRCNN_ERR_LAUNCH, "%s: cannot query the device", who);
}
inline int whole_xcds(int cus) { return cus >= 8 ? (cus / 8) * 8 : 8; }

template <typename P>
struct kernel_arg {  // keeps launch_kernel's last parameter out of deduction: a derived parameter block converts to the kernel's
    using type = P;
};
template <typename P>
int launch_kernel(void (*kern)(P), long long grid, int threads, size_t lds_bytes, hipStream_t stream, const char* who,
                  const char* kernel_name, const typename kernel_arg<P>::type& p) {
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds_bytes, who)) return rc;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(threads), lds_bytes, stream, p);
    return check_launch(kernel_name);
}
// The grid rule of the Winograd and fused-Bottleneck kernels: one workgroup per CU of the whole XCDs, fewer when there are
// fewer `units` of work; a workgroup walks the units beyond its own.
template <typename P>
int launch_one_per_cu(void (*kern)(P), long long units, int threads, size_t lds_bytes, hipStream_t stream, const char* who,
                      const char* kernel_name, const typename kernel_arg<P>::type& p) {
    int cus;
    if (int rc = query_cus(who, cus)) return rc;
    return launch_kernel(kern, std::min<long long>(units, whole_xcds(cus)), threads, lds_bytes, stream, who, kernel_name, p);
}

// Tuning switches of the launch paths (tile overrides, kernel A/B routes): environment variables honoured ONLY in -DMRCNN_TUNING
// builds (`build.py --variant tuning -DMRCNN_TUNING`, which tools/ load through MRCNN_LIB); the product library ignores them —
// it reads three variables in all: MRCNN_CROP_STAGED, MRCNN_WINO_SPATIAL (documented modes) and MRCNN_CONV_NO_SPLIT (numerics A/B).
inline const char* tuning_env(const char* name) {
#ifdef MRCNN_TUNING
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

}  // namespace mrcnn

// Schedule fuzzing (-DMRCNN_SYNC_FUZZ: an experiment build, `build.py --variant sync_fuzz -DMRCNN_SYNC_FUZZ`; never the product).
// Behind EVERY workgroup barrier each wave sleeps for a pseudo-random 0 .. 24 576 cycles. A kernel whose LDS hand-offs are
// ordered by its barriers and counted waits computes the same bits at any skew; one that is protected only by "the other
// waves cannot be that far ahead" (round 5's conv3x3_wino4_f32: ten MFMA slots stood in for a barrier) goes wrong on every
// launch instead of one in 5 000. tests/test_gpu_sync_fuzz.py runs the kernels' parity tests on such a build.
// The fuzz points: __syncthreads(), __syncthreads_or(), __syncthreads_and() and __syncthreads_count() are wrapped by the macros
// below; MRCNN_SYNC_FUZZ_POINT() follows every hand-written barrier (asm s_barrier / __builtin_amdgcn_s_barrier), in the same
// statement, macro or body. A barrier of any other form is not fuzzed: tests/test_host.py reads the sources and refuses one,
// and takes the set of wrapped names from the #define lines of this block.
#ifdef MRCNN_SYNC_FUZZ
namespace mrcnn {
__device__ __forceinline__ void sync_fuzz_point() {
    // ONE asm statement, three scalar registers, no control flow the compiler can see (the hand-scheduled kernels have no
    // vector register to spare, and a visible loop in their epilogues changes their register allocation): six bits of the
    // shader clock, a different bit window per SIMD (HW_ID.simd_id: the waves leave the barrier at the same instant), are
    // shifted out one by one with 4 096 cycles of sleep each — 0 .. 24 576 cycles, half of the waves more than 20 000.
    unsigned long long t;
    unsigned r;
    asm volatile("s_memtime %0\n\t"
                 "s_getreg_b32 %1, hwreg(HW_REG_HW_ID, 4, 2)\n\t"
                 "s_waitcnt lgkmcnt(0)\n\t"
                 "s_lshl_b32 %1, %1, 1\n\t"
                 "s_add_u32 %1, %1, 3\n\t"
                 "s_lshr_b64 %0, %0, %1\n\t"
                 "s_and_b64 %0, %0, 63\n\t"
                 "1:\n\t"
                 "s_cmp_eq_u64 %0, 0\n\t"
                 "s_cbranch_scc1 2f\n\t"
                 "s_sleep 64\n\t"
                 "s_lshr_b64 %0, %0, 1\n\t"
                 "s_branch 1b\n\t"
                 "2:"
                 : "=&s"(t), "=&s"(r)
                 :
                 : "scc", "memory");
}
__device__ __forceinline__ void fuzzed_syncthreads() {
    __syncthreads();
    sync_fuzz_point();
}
// The voting barriers (HIP's __device__ inline functions, reached here under their own names: the macros come below). The
// sleep follows the whole vote, so the waves leave it skewed as they leave a plain barrier.
__device__ __forceinline__ int fuzzed_syncthreads_or(int predicate) {
    const int r = __syncthreads_or(predicate);
    sync_fuzz_point();
    return r;
}
__device__ __forceinline__ int fuzzed_syncthreads_and(int predicate) {
    const int r = __syncthreads_and(predicate);
    sync_fuzz_point();
    return r;
}
__device__ __forceinline__ int fuzzed_syncthreads_count(int predicate) {
    const int r = __syncthreads_count(predicate);
    sync_fuzz_point();
    return r;
}
}  // namespace mrcnn
#define MRCNN_SYNC_FUZZ_POINT() ::mrcnn::sync_fuzz_point()
#define __syncthreads() ::mrcnn::fuzzed_syncthreads()
#define __syncthreads_or(predicate) ::mrcnn::fuzzed_syncthreads_or(predicate)
#define __syncthreads_and(predicate) ::mrcnn::fuzzed_syncthreads_and(predicate)
#define __syncthreads_count(predicate) ::mrcnn::fuzzed_syncthreads_count(predicate)
#else
#define MRCNN_SYNC_FUZZ_POINT() ((void)0)
#endif

#define MRCNN_REQUIRE(cond, ...)                                              \
    do {                                                                      \
        if (!(cond)) return ::mrcnn::fail(MRCNN_ERR_INVALID_ARGUMENT, __VA_ARGS__); \
    } while (0)
