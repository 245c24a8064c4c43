// BatchNorm training kernels, NHWC bf16 activations, fp32 statistics:
// statistics (+ finalize, partial fold), fused apply (+ residual, + ReLU /
// ReLU6 with a 1-bit gradient mask), backward reductions and backward dx.
//
// These ops are HBM-bound — the levers are vectorized 16-B bf16x8 accesses,
// pass fusion (BN+ReLU+residual in one read/write of the activation) and
// fp32 accumulation. All row kernels use the fixed-channel-column geometry
// of column.h.
#include "column.h"

// ---------------------------------------------------------------------------
// BatchNorm training statistics: per-channel sum / sumsq over rows = N*H*W.
// x viewed as [rows][C]; C % 8 == 0. Each thread owns 8 consecutive channels
// (one bf16x8 vector); thread groups stack over rows; LDS reduce across
// row groups; each block writes its PARTIAL sums to part[blockIdx.y][C]
// (no atomics — fp32 atomicAdd contention on the small per-channel arrays
// measured 3.5x off the HBM roofline — and fully deterministic); the
// finalize kernel reduces the <=BN_MAX_PARTS partials.
// ---------------------------------------------------------------------------
#define BN_MAX_PARTS 512  // 2 blocks/CU of 256 threads = 8 waves/CU in flight

__global__ __launch_bounds__(256) void k_bn_stats(
    const bf16_t* __restrict__ x, float* __restrict__ part_sum,
    float* __restrict__ part_sumsq, long rows, int C) {
  const ColumnGeom cg(C);
  const int vec = cg.vec(), rowg = cg.rowg();
  // inactive threads still reach every barrier (no early return!)
  const bool active = cg.active();

  float s[8] = {0}, q[8] = {0};
  const long row0 = (long)blockIdx.y * cg.ROWG + rowg;
  const long rstride = (long)gridDim.y * cg.ROWG;
  if (active) {
    long r = row0;
    for (; r + rstride < rows; r += 2 * rstride) {
      bf16x8 v0, v1;  // two independent strided loads in flight (MLP)
      v0.v = *reinterpret_cast<const uint4*>(x + r * C + (long)vec * 8);
      v1.v = *reinterpret_cast<const uint4*>(x + (r + rstride) * C + (long)vec * 8);
      #pragma unroll
      for (int k = 0; k < 8; ++k) {
        float f0 = b2f(v0.h[k]), f1 = b2f(v1.h[k]);
        s[k] += f0 + f1;
        q[k] += f0 * f0 + f1 * f1;
      }
    }
    if (r < rows) {
      bf16x8 v;
      v.v = *reinterpret_cast<const uint4*>(x + r * C + (long)vec * 8);
      #pragma unroll
      for (int k = 0; k < 8; ++k) {
        float f = b2f(v.h[k]);
        s[k] += f;
        q[k] += f * f;
      }
    }
  }
  // reduce across row groups through LDS
  __shared__ float lds[256 * 8];
  if (cg.ROWG > 1) {                            // block-uniform
    rowgroup_reduce8(cg, lds, s);
    __syncthreads();
    rowgroup_reduce8(cg, lds, q);
  }
  if (active && rowg == 0) {
    float* ps = part_sum + (long)blockIdx.y * C;
    float* pq = part_sumsq + (long)blockIdx.y * C;
    #pragma unroll
    for (int k = 0; k < 8; ++k) {
      ps[vec * 8 + k] = s[k];
      pq[vec * 8 + k] = q[k];
    }
  }
}

// finalize: reduce partials -> mean/rstd + running-stat update (K4).
// Block = 32 channels x 8 part-groups (a one-thread-per-channel loop over
// up to 512 strided partials measured 128 us — pure load latency); each
// thread sums parts pg::8 (coalesced across the 32 channel lanes), LDS
// tree over the 8 groups, group 0 finishes the math.
__global__ __launch_bounds__(256) void k_bn_finalize(
    const float* __restrict__ part_sum, const float* __restrict__ part_sumsq,
    float* __restrict__ mean, float* __restrict__ rstd,
    float* __restrict__ running_mean, float* __restrict__ running_var,
    long rows, int C, int nparts, float eps, float momentum) {
  const int cl = threadIdx.x & 31;
  const int pg = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float s = 0.f, q = 0.f;
  if (c < C) {
    for (int p = pg; p < nparts; p += 8) {
      s += part_sum[(long)p * C + c];
      q += part_sumsq[(long)p * C + c];
    }
  }
  __shared__ float ls[8][32], lq[8][32];
  ls[pg][cl] = s;
  lq[pg][cl] = q;
  __syncthreads();
  if (pg == 0 && c < C) {
    #pragma unroll
    for (int g = 1; g < 8; ++g) {
      s += ls[g][cl];
      q += lq[g][cl];
    }
    float m = s / (float)rows;
    float var = fmaxf(q / (float)rows - m * m, 0.f);
    mean[c] = m;
    rstd[c] = rsqrtf(var + eps);
    if (running_mean) {
      float unbiased = var * (float)rows / (float)(rows > 1 ? rows - 1 : 1);
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
    }
  }
}

// ---------------------------------------------------------------------------
// BN apply (+ optional residual add, + optional ReLU), one fused pass:
//   y = act((x - mean[c]) * rstd[c] * gamma[c] + beta[c] [+ res])
// RELU: 0 = identity, 1 = relu, 2 = relu6 (mask bit = "gradient passes",
// so the backward kernels take a relu6 layer as RELU = 1). res may be null.
// ---------------------------------------------------------------------------
// Geometry (shared with k_bn_bwd_dx): each thread owns ONE fixed 8-channel
// vector column and streams rows, so the per-channel tables are loaded ONCE
// into registers and folded (y = x*scale + shift) — the naive grid-stride
// form reloads 4 tables x 8 scalars per 16-B vector (issue-bound, measured
// 1.6x off the HBM roofline on the 56^2 layers).
template <int RELU, bool HAS_RES>
__global__ __launch_bounds__(256) void k_bn_apply(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ res,
    bf16_t* __restrict__ y, unsigned char* __restrict__ mask,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    long rows, int C) {
  const ColumnGeom cg(C);
  const int vecC = cg.vecC, ROWG = cg.ROWG;
  const int vec = cg.vec(), rowg = cg.rowg();
  if (!cg.active()) return;                     // no barrier below
  float scale[8], shift[8];
  #pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = vec * 8 + k;
    scale[k] = rstd[c] * gamma[c];
    shift[k] = beta[c] - mean[c] * scale[k];
  }
  const long rstride = (long)gridDim.y * ROWG;
  auto body = [&](long r) {
    const long base = r * C + (long)vec * 8;
    bf16x8 v, o, rv;
    v.v = *reinterpret_cast<const uint4*>(x + base);
    if (HAS_RES) rv.v = *reinterpret_cast<const uint4*>(res + base);
    unsigned char mb = 0;
    #pragma unroll
    for (int k = 0; k < 8; ++k) {
      float f = b2f(v.h[k]) * scale[k] + shift[k];
      if (HAS_RES) f += b2f(rv.h[k]);
      if (RELU == 2) {
        // ReLU6: gradient passes iff 0 < f < 6, decided on the fp32 value
        // before bf16 rounding (hardtanh_backward's rule)
        if (f > 0.f && f < 6.f) mb |= (1u << k);
        f = fminf(fmaxf(f, 0.f), 6.f);
      } else if (RELU) {
        if (f > 0.f) mb |= (1u << k);
        f = fmaxf(f, 0.f);
      }
      o.h[k] = f2b(f);
    }
    *reinterpret_cast<uint4*>(y + base) = o.v;
    if (RELU) mask[r * vecC + vec] = mb;  // 1 byte per 8-channel vector:
                                          // bwd reads this instead of y
  };
  // 2x row unroll: two independent strided streams per thread keeps more
  // loads in flight (single 16-B load/thread was MLP-starved)
  long r = (long)blockIdx.y * ROWG + rowg;
  for (; r + rstride < rows; r += 2 * rstride) {
    body(r);
    body(r + rstride);
  }
  if (r < rows) body(r);
}

// ---------------------------------------------------------------------------
// BN backward reductions: with fused ReLU the incoming dy must be masked by
// (y > 0) first; we take y (the saved activation output) and produce
//   dbeta[c]  = sum(dy_m),  dgamma[c] = sum(dy_m * xhat)
// Same thread geometry as k_bn_stats.
// ---------------------------------------------------------------------------
template <int RELU>
__global__ __launch_bounds__(256) void k_bn_bwd_reduce(
    const bf16_t* __restrict__ dy, const unsigned char* __restrict__ mask,
    const bf16_t* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ dbeta, float* __restrict__ dgamma,
    long rows, int C) {
  const ColumnGeom cg(C);
  const int vecC = cg.vecC, ROWG = cg.ROWG;
  const int vec = cg.vec(), rowg = cg.rowg();
  const bool active = cg.active();              // idle threads reach the barriers

  float db[8] = {0}, dg[8] = {0};
  float mn[8], rs[8];
  if (active) {
    #pragma unroll
    for (int k = 0; k < 8; ++k) { mn[k] = mean[vec * 8 + k]; rs[k] = rstd[vec * 8 + k]; }
    const long row0 = (long)blockIdx.y * ROWG + rowg;
    const long rstride = (long)gridDim.y * ROWG;
    // (2x unroll measured slower here — two dy+x+mask streams thrash;
    // the read-only stats kernel keeps its unroll, this one stays simple)
    for (long r = row0; r < rows; r += rstride) {
      const long base = r * C + (long)vec * 8;
      bf16x8 vdy, vx;
      vdy.v = *reinterpret_cast<const uint4*>(dy + base);
      vx.v = *reinterpret_cast<const uint4*>(x + base);
      unsigned char mb = RELU ? mask[r * vecC + vec] : 0xff;
      #pragma unroll
      for (int k = 0; k < 8; ++k) {
        float g = b2f(vdy.h[k]);
        if (RELU && !((mb >> k) & 1)) g = 0.f;
        db[k] += g;
        dg[k] += g * (b2f(vx.h[k]) - mn[k]) * rs[k];
      }
    }
  }
  __shared__ float lds[256 * 8];
  if (ROWG > 1) {                               // block-uniform
    rowgroup_reduce8(cg, lds, db);
    __syncthreads();
    rowgroup_reduce8(cg, lds, dg);
  }
  if (active && rowg == 0) {
    float* pb = dbeta + (long)blockIdx.y * C;   // partial rows, finalized below
    float* pg = dgamma + (long)blockIdx.y * C;
    #pragma unroll
    for (int k = 0; k < 8; ++k) {
      pb[vec * 8 + k] = db[k];
      pg[vec * 8 + k] = dg[k];
    }
  }
}

// reduce the bwd partials -> dbeta[C], dgamma[C] (same geometry as above)
__global__ __launch_bounds__(256) void k_bn_grad_finalize(
    const float* __restrict__ part_db, const float* __restrict__ part_dg,
    float* __restrict__ dbeta, float* __restrict__ dgamma, int C, int nparts) {
  const int cl = threadIdx.x & 31;
  const int pg = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float b = 0.f, g = 0.f;
  if (c < C) {
    for (int p = pg; p < nparts; p += 8) {
      b += part_db[(long)p * C + c];
      g += part_dg[(long)p * C + c];
    }
  }
  __shared__ float lb[8][32], lg[8][32];
  lb[pg][cl] = b;
  lg[pg][cl] = g;
  __syncthreads();
  if (pg == 0 && c < C) {
    #pragma unroll
    for (int gg = 1; gg < 8; ++gg) {
      b += lb[gg][cl];
      g += lg[gg][cl];
    }
    dbeta[c] = b;
    dgamma[c] = g;
  }
}

// ---------------------------------------------------------------------------
// BN backward dx (+ optional residual grad out):
//   dy_m = RELU ? dy * (y > 0) : dy
//   dx   = gamma*rstd * (dy_m - dbeta/M - xhat * dgamma/M)
//   dres = dy_m (residual branch gets the masked upstream grad)
// ---------------------------------------------------------------------------
// Same fixed-channel geometry as k_bn_apply; the per-channel terms fold to
//   dx = A*dy_m - B*x + D   with A = gamma*rstd, B = A*rstd*dgamma/M,
//   D = -A*dbeta/M + B*mean  (2 FMA per element, tables in registers).
template <int RELU, bool HAS_RES>
__global__ __launch_bounds__(256) void k_bn_bwd_dx(
    const bf16_t* __restrict__ dy, const unsigned char* __restrict__ mask,
    const bf16_t* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma,
    const float* __restrict__ dbeta, const float* __restrict__ dgamma,
    bf16_t* __restrict__ dx, bf16_t* __restrict__ dres,
    long rows, int C) {
  const ColumnGeom cg(C);
  const int vecC = cg.vecC, ROWG = cg.ROWG;
  const int vec = cg.vec(), rowg = cg.rowg();
  if (!cg.active()) return;                     // no barrier below
  const float invM = 1.f / (float)rows;
  float A[8], B[8], D[8];
  #pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = vec * 8 + k;
    A[k] = gamma[c] * rstd[c];
    B[k] = A[k] * rstd[c] * dgamma[c] * invM;
    D[k] = B[k] * mean[c] - A[k] * dbeta[c] * invM;
  }
  const long rstride = (long)gridDim.y * ROWG;
  auto body = [&](long r) {
    const long base = r * C + (long)vec * 8;
    bf16x8 vdy, vx, odx, odr;
    vdy.v = *reinterpret_cast<const uint4*>(dy + base);
    vx.v = *reinterpret_cast<const uint4*>(x + base);
    const unsigned char mb = RELU ? mask[r * vecC + vec] : 0xff;
    #pragma unroll
    for (int k = 0; k < 8; ++k) {
      float g = b2f(vdy.h[k]);
      if (RELU && !((mb >> k) & 1)) g = 0.f;
      float d = A[k] * g - B[k] * b2f(vx.h[k]) + D[k];
      odx.h[k] = f2b(d);
      if (HAS_RES) odr.h[k] = f2b(g);
    }
    *reinterpret_cast<uint4*>(dx + base) = odx.v;
    if (HAS_RES) *reinterpret_cast<uint4*>(dres + base) = odr.v;
  };
  long r = (long)blockIdx.y * ROWG + rowg;
  for (; r + rstride < rows; r += 2 * rstride) {
    body(r);
    body(r + rstride);
  }
  if (r < rows) body(r);
}

// Fold a LARGE partial set (conv-epilogue fused stats: nparts = grid_m x
// waves_m, up to ~12k rows) down to G rows with a chip-filling grid —
// k_bn_finalize's grid is only ceil(C/32) blocks (2 for C=64) and would
// serialize the strided reads of a 12k-row partial buffer on 2 CUs.
__global__ __launch_bounds__(256) void k_bn_parts_fold(
    const float* __restrict__ ps, const float* __restrict__ pq,
    float* __restrict__ os, float* __restrict__ oq, long nparts, int C,
    int G) {
  const int cl = threadIdx.x & 31;
  const int pg = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const int g = blockIdx.y;
  float s = 0.f, q = 0.f;
  if (c < C) {
    for (long p = (long)g * 8 + pg; p < nparts; p += (long)G * 8) {
      s += ps[p * C + c];
      q += pq[p * C + c];
    }
  }
  __shared__ float ls[8][32], lq[8][32];
  ls[pg][cl] = s;
  lq[pg][cl] = q;
  __syncthreads();
  if (pg == 0 && c < C) {
    #pragma unroll
    for (int i = 1; i < 8; ++i) {
      s += ls[i][cl];
      q += lq[i][cl];
    }
    os[(long)g * C + c] = s;
    oq[(long)g * C + c] = q;
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// grid of the two row reductions; grid.y (= partial count) must match
// between the reduce launch and its finalize
static inline dim3 bn_reduce_grid(long rows, int C) {
  const ColumnGeom cg(C);
  return dim3(cg.gx, cg.reduce_slices(rows, BN_MAX_PARTS));
}

DDLW_EXPORT int ddlw_bn_nparts(long rows, int C) {
  return ColumnGeom(C).reduce_slices(rows, BN_MAX_PARTS);
}

DDLW_EXPORT int ddlw_bn_stats(const void* x, void* part_sum, void* part_sumsq,
                              long rows, int C, void* stream) {
  dim3 grid = bn_reduce_grid(rows, C);
  hipLaunchKernelGGL(k_bn_stats, grid, dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, (float*)part_sum, (float*)part_sumsq,
                     rows, C);
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_bn_parts_fold(const void* ps, const void* pq, void* os,
                                   void* oq, long nparts, int C, int G,
                                   void* stream) {
  dim3 grid((C + 31) / 32, G);
  hipLaunchKernelGGL(k_bn_parts_fold, grid, dim3(256), 0, (hipStream_t)stream,
                     (const float*)ps, (const float*)pq, (float*)os,
                     (float*)oq, nparts, C, G);
  DDLW_CHECK_LAUNCH();
}

// finalize over the caller's partial count: ddlw_bn_nparts(rows, C) after
// ddlw_bn_stats, grid_m * waves_m (or the fold's G) after conv-epilogue
// fused stats
DDLW_EXPORT int ddlw_bn_finalize(const void* part_sum, const void* part_sumsq,
                                 void* mean, void* rstd, void* rmean,
                                 void* rvar, long rows, int C, int nparts,
                                 float eps, float momentum, void* stream) {
  hipLaunchKernelGGL(k_bn_finalize, dim3((C + 31) / 32), dim3(256), 0,
                     (hipStream_t)stream, (const float*)part_sum,
                     (const float*)part_sumsq, (float*)mean, (float*)rstd,
                     (float*)rmean, (float*)rvar, rows, C, nparts, eps,
                     momentum);
  DDLW_CHECK_LAUNCH();
}

// grid for the fixed-channel elementwise BN kernels: x covers channel-vector
// groups, y covers row groups (capped; kernels stride the remainder)
static inline dim3 bn_ew_grid(long rows, int C) {
  const ColumnGeom cg(C);
  return dim3(cg.gx, cg.capped_slices(rows, 4096));
}

DDLW_EXPORT int ddlw_bn_apply(const void* x, const void* res, void* y,
                              void* mask, const void* mean, const void* rstd,
                              const void* gamma, const void* beta, long rows,
                              int C, int relu, void* stream) {
  dim3 grid = bn_ew_grid(rows, C);
  with_int<2, 0, 1>(relu, [&](auto RELU) {  // any other nonzero mode = ReLU
    with_bool(res != nullptr, [&](auto RES) {
      hipLaunchKernelGGL((k_bn_apply<decltype(RELU)::value, decltype(RES)::value>),
                         grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                         (const bf16_t*)res, (bf16_t*)y, (unsigned char*)mask,
                         (const float*)mean, (const float*)rstd,
                         (const float*)gamma, (const float*)beta, rows, C);
    });
  });
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_bn_bwd_reduce(const void* dy, const void* mask, const void* x,
                                   const void* mean, const void* rstd,
                                   void* dbeta, void* dgamma, long rows, int C,
                                   int relu, void* stream) {
  dim3 grid = bn_reduce_grid(rows, C);
  with_int<0, 1>(relu, [&](auto RELU) {
    hipLaunchKernelGGL((k_bn_bwd_reduce<decltype(RELU)::value>), grid,
                       dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy,
                       (const unsigned char*)mask, (const bf16_t*)x,
                       (const float*)mean, (const float*)rstd, (float*)dbeta,
                       (float*)dgamma, rows, C);
  });
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_bn_grad_finalize(const void* part_db, const void* part_dg,
                                      void* dbeta, void* dgamma, int C,
                                      int nparts, void* stream) {
  hipLaunchKernelGGL(k_bn_grad_finalize, dim3((C + 31) / 32), dim3(256), 0,
                     (hipStream_t)stream, (const float*)part_db,
                     (const float*)part_dg, (float*)dbeta, (float*)dgamma, C,
                     nparts);
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_bn_bwd_dx(const void* dy, const void* mask, const void* x,
                               const void* mean, const void* rstd,
                               const void* gamma, const void* dbeta,
                               const void* dgamma, void* dx, void* dres,
                               long rows, int C, int relu, void* stream) {
  dim3 grid = bn_ew_grid(rows, C);
  with_int<0, 1>(relu, [&](auto RELU) {
    with_bool(dres != nullptr, [&](auto DRES) {
      hipLaunchKernelGGL((k_bn_bwd_dx<decltype(RELU)::value, decltype(DRES)::value>),
                         grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy,
                         (const unsigned char*)mask, (const bf16_t*)x,
                         (const float*)mean, (const float*)rstd,
                         (const float*)gamma, (const float*)dbeta,
                         (const float*)dgamma, (bf16_t*)dx, (bf16_t*)dres,
                         rows, C);
    });
  });
  DDLW_CHECK_LAUNCH();
}
