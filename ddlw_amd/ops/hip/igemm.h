// Shared pieces of the implicit-GEMM convolution files (conv_gemm.hip,
// conv_wgrad.hip, conv_stem.hip).
#pragma once
#include "common.h"

// address spaces of the global_load_lds builtin's operands
#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

// host-precomputed magic division (Granlund-Montgomery): q = (m*M) >> (64)
// ... here the (32+s)-shift variant; valid for the m < 2^31 row indices.
// Avoids the ~100-cycle 64-bit div/mod expansion per thread in the prologue
// (dominant on 1-k-step shapes).
__device__ __forceinline__ unsigned mdiv(unsigned m, unsigned long long magic,
                                         unsigned shift) {
  return (unsigned)(((unsigned long long)m * magic) >> shift);
}

// ceil-magic for q = m/d exact for all m < 2^31:
// s = ceil(log2 d); magic = ceil(2^(32+s) / d); q = (m*magic) >> (32+s)
static inline void make_magic(unsigned d, unsigned long long* magic, unsigned* shift) {
  if (d == 1) { *magic = 1ull << 32; *shift = 32; return; }
  unsigned s = 0;
  while ((1ull << s) < d) ++s;
  *magic = ((1ull << (32 + s)) + d - 1) / d;
  *shift = 32 + s;
}

// fp32 split slabs -> bf16 dW; defined in conv_wgrad.hip, also launched by
// the stem wgrad
__global__ __launch_bounds__(256) void k_wgrad_reduce(
    const float* __restrict__ slab, bf16_t* __restrict__ dw, long elems, int split);
