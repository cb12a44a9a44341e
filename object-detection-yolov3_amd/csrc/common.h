// Shared helpers for the gfx950 kernels of libyolo3hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include "host.h"   // error channel, Y3_CHECK_ARG, integer helpers, Y3Div: everything that needs no HIP

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define Y3_CHECK_LAUNCH(what)                                              \
    do {                                                                   \
        hipError_t e_ = hipGetLastError();                                 \
        if (e_ != hipSuccess) {                                            \
            y3_set_error("%s: %s", what, hipGetErrorString(e_));          \
            return Y3_ELAUNCH;                                             \
        }                                                                  \
    } while (0)

// grid of a streaming kernel with a grid-stride loop (pointwise.hip, optim.hip): one thread per item, capped at ~8 blocks/CU
static inline int stream_blocks(long long items, int threads) {
    long long b = (items + threads - 1) / threads;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

// Blocks are dealt round-robin over the 8 XCDs (each with a private L2): remap so
// that every XCD works on one contiguous run of tile ids (bijective for any grid).
__device__ __forceinline__ int y3_xcd_remap(int orig, int nwg) {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = orig & 7, j = orig >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}

// Workgroup barrier that orders LDS traffic only: global loads issued before it stay in flight across it (a plain
// __syncthreads() also waits for vmcnt(0)).
__device__ __forceinline__ void y3_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ float y3_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double y3_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int y3_div(int x, const Y3Div d) { return d.mul ? (int)(__umulhi((unsigned)x, d.mul) >> d.shift) : x; }
#define Y3_PIN_S(x) asm volatile("" : "+s"(x))

