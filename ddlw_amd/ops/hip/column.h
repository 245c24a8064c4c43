// Fixed-channel-column geometry of the per-channel row kernels (BN stats /
// apply / backward, depthwise wgrad). x is viewed as [rows][C], C % 8 == 0.
// A block of 256 threads covers VPB 8-channel vectors x ROWG row groups: each
// thread owns ONE vector column and strides over rows, so per-channel tables
// live in registers. grid.x covers the vectors, grid.y slices the rows.
// Kernel and launcher both build this struct, because the slice count of a
// reduction is part of its result (it fixes the summation order).
#pragma once
#include "common.h"

struct ColumnGeom {
  int vecC;  // 8-channel vectors per row
  int VPB;   // vectors per block
  int ROWG;  // row groups per block (floor: 256 % VPB threads stay idle)
  int gx;    // grid.x

  __host__ __device__ __forceinline__ explicit ColumnGeom(int C) {  // C >= 8
    vecC = C >> 3;
    VPB = vecC < 256 ? vecC : 256;
    ROWG = 256 / VPB;
    gx = (vecC + VPB - 1) / VPB;
  }

  // this thread's place in the block
  __device__ __forceinline__ int lane_vec() const { return (int)threadIdx.x % VPB; }
  __device__ __forceinline__ int vec() const { return blockIdx.x * VPB + lane_vec(); }
  __device__ __forceinline__ int rowg() const { return (int)threadIdx.x / VPB; }
  __device__ __forceinline__ bool active() const {
    return (rowg() < ROWG) && (vec() < vecC);
  }

  // grid.y of a reduction = its partial count: one slice per row-group
  // stack, at most max_parts
  int reduce_slices(long rows, int max_parts) const {
    long ny = cdiv(rows, ROWG);
    return (int)(ny < max_parts ? ny : max_parts);
  }

  // grid.y when the whole grid is held to about `cap` blocks (kernels stride
  // over the remaining rows); never below 1
  int capped_slices(long rows, int cap) const {
    long need = cdiv(rows, ROWG);
    long most = cap / gx;
    if (most < 1) most = 1;
    long gy = need < most ? need : most;
    return (int)(gy < 1 ? 1 : gy);
  }
};

// Sum one float[8] per thread across the ROWG row groups of a block through
// lds[256 * 8]: every thread stores at lds[tid * 8 + k], one barrier, then
// row group 0 adds groups 1..ROWG-1 in ascending order (fixed order: the
// result does not depend on scheduling). Called by ALL 256 threads, idle ones
// included. Reusing lds afterwards needs another barrier first.
__device__ __forceinline__ void rowgroup_reduce8(const ColumnGeom& cg, float* lds,
                                                 float (&v)[8]) {
  const int tid = threadIdx.x;
  #pragma unroll
  for (int k = 0; k < 8; ++k) lds[tid * 8 + k] = v[k];
  __syncthreads();
  if (cg.rowg() == 0) {
    // summed in a local copy: accumulating through the reference makes the
    // compiler emit ~20% more code for the same sums in the BN reductions
    float a[8];
    #pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = v[k];
    for (int g = 1; g < cg.ROWG; ++g)
      #pragma unroll
      for (int k = 0; k < 8; ++k) a[k] += lds[(g * cg.VPB + cg.lane_vec()) * 8 + k];
    #pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = a[k];
  }
}
