// Common helpers for ddlw CDNA4 (gfx950) kernels.
// Layout convention: activations are NHWC bf16 (torch channels_last);
// statistics/parameters are fp32. All reductions accumulate in fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <type_traits>

#define DDLW_EXPORT extern "C" __attribute__((visibility("default")))

typedef unsigned short bf16_t;
typedef unsigned int u32;
typedef unsigned long long u64;

// 8 bf16 = one 16-byte vector load (guideline: vectorize bf16 as short8)
union bf16x8 {
  uint4 v;
  bf16_t h[8];
};

__device__ __forceinline__ float b2f(bf16_t h) {
  union { float f; u32 u; } cvt;
  cvt.u = ((u32)h) << 16;
  return cvt.f;
}

__device__ __forceinline__ bf16_t f2b(float f) {
  // hardware RNE convert (v_cvt path; same rounding as the manual
  // integer-bias form but ~1 VALU instead of ~5)
  __bf16 h = (__bf16)f;
  union { __bf16 h; bf16_t u; } cvt;
  cvt.h = h;
  return cvt.u;
}

__device__ __forceinline__ float warp_reduce_sum(float v) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ float warp_reduce_max(float v) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  return v;
}

// Sum over the 16 lanes of a DPP row (lane & 15 = the 16 rows of an MFMA
// fragment, or 16 pixels): rotate by 8, 4, 2, 1 within the row. Every lane
// ends with the total, added in an order that depends on nothing but the lane.
template <int CTRL>
__device__ __forceinline__ float row_ror_add(float v) {
  const int i = __float_as_int(v);
  return v + __int_as_float(__builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ float row_sum16(float v) {
  v = row_ror_add<0x128>(v);  // row_ror:8
  v = row_ror_add<0x124>(v);  // row_ror:4
  v = row_ror_add<0x122>(v);  // row_ror:2
  return row_ror_add<0x121>(v);  // row_ror:1
}

// 8 consecutive fp32 (a per-channel table slice) as two 16-byte loads
__device__ __forceinline__ void load8f(const float* __restrict__ p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// fused activation epilogue: 0 none, 1 ReLU, 2 ReLU6
__device__ __forceinline__ float apply_act(float v, int act) {
  if (act >= 1) v = fmaxf(v, 0.f);
  if (act == 2) v = fminf(v, 6.f);
  return v;
}

// Conv tap index clamped into [0, hi]: an out-of-range tap loads from this
// (always valid) address and the loaded vector is zeroed afterwards, so the
// tap loads of a pixel issue back to back with no branch between them.
__device__ __forceinline__ int clamp_tap(int v, int hi) {
  return v < 0 ? 0 : (v > hi ? hi : v);
}

// launch geometry -----------------------------------------------------------
static inline long cdiv(long a, long b) { return (a + b - 1) / b; }

// 1-D grid for a grid-stride kernel: ceil(work / block), at least 1, capped
static inline int grid_1d(long work, int block = 256, int cap = 2048) {
  long g = cdiv(work, block);
  return (int)(g < cap ? (g > 0 ? g : 1) : cap);
}

// error plumbing (core.hip) -------------------------------------------------
#define DDLW_CHECK_LAUNCH()                                                   \
  do {                                                                         \
    hipError_t err_ = hipGetLastError();                                       \
    if (err_ != hipSuccess) {                                                  \
      ddlw_set_error(hipGetErrorString(err_));                                 \
      return 1;                                                                \
    }                                                                          \
    return 0;                                                                  \
  } while (0)

// between two launches of one export: return 1 on a launch error, else go on
#define DDLW_CHECK_LAUNCH_OR_RETURN()                                         \
  do {                                                                         \
    hipError_t err_ = hipGetLastError();                                       \
    if (err_ != hipSuccess) {                                                  \
      ddlw_set_error(hipGetErrorString(err_));                                 \
      return 1;                                                                \
    }                                                                          \
  } while (0)

void ddlw_set_error(const char* msg);
// sets the error to "who: why" and returns 2 (the bad-argument status)
int ddlw_fail(const char* who, const char* why);

// launch dispatch -----------------------------------------------------------
// Runtime value -> template argument: f is a generic lambda that receives a
// std::integral_constant, so a launch statement is written once and
// instantiated per listed value. with_int falls back to the LAST listed value.
template <class F>
static inline void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

template <int V, int... Rest, class F>
static inline void with_int(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) {
    f(std::integral_constant<int, V>{});
  } else {
    if (v == V) f(std::integral_constant<int, V>{});
    else with_int<Rest...>(v, f);
  }
}
