// Depthwise conv2d (K2 — MobileNetV2's depthwise blocks), NHWC bf16, fp32
// accumulation: training forward, eval forward with the folded-BN epilogue,
// and the 3x3 backward (dgrad, wgrad + finalize).
// Data conventions of the whole family: C % 8 == 0, 16-byte bf16x8 accesses,
// weights pre-transposed host-side to [R*S][C] so the per-tap weight read is
// the same contiguous vector shape as the activation read.
//
// Every direction is memory-bound. All kernels but k_depthwise_fwd handle
// out-of-range taps by loading from a CLAMPED (always valid) address and
// zeroing the vector afterwards (clamp_tap), so every tap load of a pixel is
// issued back to back with no branch (and no wait) between them.
#include "column.h"

#define DW_K 3               // kernel extent of the 3x3-only kernels
#define DW_MAX_PARTS 512     // row-slice partials of the wgrad (2 blocks/CU)

// ---------------------------------------------------------------------------
// Training forward, any R x S and stride: one thread per 8-channel vector of
// one output pixel, out-of-range taps skipped by a branch.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_depthwise_fwd(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w_t,
    bf16_t* __restrict__ y, int N, int H, int W_, int C, int Ho, int Wo,
    int R, int S, int stride, int pad) {
  const int vecC = C >> 3;
  const long total = (long)N * Ho * Wo * vecC;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    int vc = (int)(i % vecC);
    long t = i / vecC;
    int wo = (int)(t % Wo); t /= Wo;
    int ho = (int)(t % Ho); t /= Ho;
    int n = (int)t;
    const int hb = ho * stride - pad, wb = wo * stride - pad;
    float acc[8] = {0};
    for (int r = 0; r < R; ++r) {
      int h = hb + r;
      if (h < 0 || h >= H) continue;
      for (int s = 0; s < S; ++s) {
        int ww = wb + s;
        if (ww < 0 || ww >= W_) continue;
        bf16x8 vx, vw;
        vx.v = *reinterpret_cast<const uint4*>(
            x + (((long)n * H + h) * W_ + ww) * C + (long)vc * 8);
        vw.v = *reinterpret_cast<const uint4*>(
            w_t + ((long)r * S + s) * C + (long)vc * 8);
        #pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += b2f(vx.h[k]) * b2f(vw.h[k]);
      }
    }
    bf16x8 o;
    #pragma unroll
    for (int k = 0; k < 8; ++k) o.h[k] = f2b(acc[k]);
    *reinterpret_cast<uint4*>(y + i * 8) = o.v;
  }
}

// ---------------------------------------------------------------------------
// Eval forward, 3x3, with the frozen model's folded-BN epilogue (the one
// k_pw_conv applies): y = act(dw(x)*scale[c]+bias[c]), act 0 none, 1 ReLU,
// 2 ReLU6. k_depthwise_fwd's thread mapping with clamped taps.
// ---------------------------------------------------------------------------
template <int STRIDE>
__global__ __launch_bounds__(256) void k_depthwise_fwd_ep(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w_t,
    bf16_t* __restrict__ y, const float* __restrict__ scale,
    const float* __restrict__ bias, int act, int N, int H, int W_, int C,
    int Ho, int Wo, int pad) {
  const int vecC = C >> 3;
  const long total = (long)N * Ho * Wo * vecC;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int vc = (int)(i % vecC);
    long t = i / vecC;
    const int wo = (int)(t % Wo); t /= Wo;
    const int ho = (int)(t % Ho); t /= Ho;
    const long n = t;
    const int hb = ho * STRIDE - pad, wb = wo * STRIDE - pad;
    float acc[8] = {0};
    // one tap row (3 x + 3 w vectors) in flight at a time: with all nine taps
    // unrolled the 18 live vectors cost 138 VGPRs = 3 waves/SIMD, and on
    // this memory-bound kernel occupancy hides more latency than issue order
    #pragma unroll 1
    for (int r = 0; r < 3; ++r) {
      const int h = hb + r;
      const bool okr = (h >= 0) && (h < H);
      const int hc = clamp_tap(h, H - 1);
      #pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int ww = wb + s;
        const bool ok = okr && (ww >= 0) && (ww < W_);
        const int wc = clamp_tap(ww, W_ - 1);
        bf16x8 vx, vw;
        vx.v = *reinterpret_cast<const uint4*>(
            x + ((n * H + hc) * W_ + wc) * C + (long)vc * 8);
        vw.v = *reinterpret_cast<const uint4*>(
            w_t + (long)(r * 3 + s) * C + (long)vc * 8);
        if (!ok) vx.v = make_uint4(0u, 0u, 0u, 0u);
        #pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += b2f(vx.h[k]) * b2f(vw.h[k]);
      }
    }
    float sc[8], bi[8];
    load8f(scale + vc * 8, sc);
    load8f(bias + vc * 8, bi);
    bf16x8 o;
    #pragma unroll
    for (int k = 0; k < 8; ++k) o.h[k] = f2b(apply_act(acc[k] * sc[k] + bi[k], act));
    *reinterpret_cast<uint4*>(y + i * 8) = o.v;
  }
}

// ---------------------------------------------------------------------------
// dgrad, gather form (no atomics):
//   dx[n,h,w,c] = sum_{r,s} dy[n,(h+pad-r)/st,(w+pad-s)/st,c] * w[c,r,s]
// over the taps whose division is exact and whose index is in range. One
// thread per 8-channel vector of one dx pixel; every dx vector is written
// exactly once, also the pixels no tap reaches (stride 2, odd H/W).
// Per axis only the taps r = (h+pad)%st + a*st can divide exactly, so the
// stride-2 kernel visits 2x2 candidates instead of 3x3.
// ---------------------------------------------------------------------------
template <int STRIDE>
__global__ __launch_bounds__(256) void k_depthwise_dgrad(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w_t,
    bf16_t* __restrict__ dx, int N, int H, int W_, int C, int Ho, int Wo,
    int pad) {
  constexpr int TAPS = (DW_K + STRIDE - 1) / STRIDE;
  const int vecC = C >> 3;
  const long total = (long)N * H * W_ * vecC;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int vc = (int)(i % vecC);
    long t = i / vecC;
    const int w = (int)(t % W_); t /= W_;
    const int h = (int)(t % H); t /= H;
    const long n = t;
    const int hp = h + pad, wp = w + pad;      // >= 0
    const int r0 = hp % STRIDE, s0 = wp % STRIDE;
    float acc[8] = {0};
    #pragma unroll
    for (int a = 0; a < TAPS; ++a) {
      const int r = r0 + a * STRIDE;
      const int ho = (hp - r) / STRIDE;        // exact by construction
      const bool okr = (r < DW_K) && (hp >= r) && (ho < Ho);
      const int hoc = clamp_tap(ho, Ho - 1);
      const int rc = r < DW_K ? r : DW_K - 1;
      #pragma unroll
      for (int b = 0; b < TAPS; ++b) {
        const int s = s0 + b * STRIDE;
        const int wo = (wp - s) / STRIDE;
        const bool ok = okr && (s < DW_K) && (wp >= s) && (wo < Wo);
        const int woc = clamp_tap(wo, Wo - 1);
        const int sc = s < DW_K ? s : DW_K - 1;
        bf16x8 vd, vw;
        vd.v = *reinterpret_cast<const uint4*>(
            dy + ((n * Ho + hoc) * Wo + woc) * C + (long)vc * 8);
        vw.v = *reinterpret_cast<const uint4*>(
            w_t + (long)(rc * DW_K + sc) * C + (long)vc * 8);
        if (!ok) vd.v = make_uint4(0u, 0u, 0u, 0u);
        #pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += b2f(vd.h[k]) * b2f(vw.h[k]);
      }
    }
    bf16x8 o;
    #pragma unroll
    for (int k = 0; k < 8; ++k) o.h[k] = f2b(acc[k]);
    *reinterpret_cast<uint4*>(dx + i * 8) = o.v;
  }
}

// ---------------------------------------------------------------------------
// wgrad: dw[c,r,s] = sum_{n,ho,wo} dy[n,ho,wo,c] * x[n,ho*st-pad+r,wo*st-pad+s,c]
// A per-channel reduction over rows = N*Ho*Wo output pixels — the problem
// shape of k_bn_bwd_reduce (bn.hip), and the same column geometry
// (column.h): each thread owns ONE fixed 8-channel vector column, thread
// groups stack over rows, grid.y slices the rows. A thread keeps 9 taps x 8 channels of fp32 accumulators
// in registers (every index is compile-time: the tap loops are unrolled).
// Row groups are summed through LDS in fixed order, one tap at a time, and
// each block writes one [9][C] fp32 partial. No atomics: the result does
// not depend on block scheduling.
// ---------------------------------------------------------------------------
template <int STRIDE>
__global__ __launch_bounds__(256) void k_depthwise_wgrad_part(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
    float* __restrict__ part, int N, int H, int W_, int C, int Ho, int Wo,
    int pad) {
  const ColumnGeom cg(C);
  const int ROWG = cg.ROWG;
  const int vec = cg.vec(), rowg = cg.rowg();
  // inactive threads still reach every barrier (no early return)
  const bool active = cg.active();

  float acc[DW_K * DW_K][8];
  #pragma unroll
  for (int t = 0; t < DW_K * DW_K; ++t)
    #pragma unroll
    for (int k = 0; k < 8; ++k) acc[t][k] = 0.f;

  if (active) {
    // pixel counts fit 32 bits (checked by the host entry): 32-bit index
    // math, and no unrolling across rows — with 64-bit divisions and the
    // compiler's 8x row unroll the loop body outgrew the instruction cache
    const int rows = N * Ho * Wo;
    const int rstride = (int)gridDim.y * ROWG;
    #pragma unroll 1
    for (int p = (int)blockIdx.y * ROWG + rowg; p < rows; p += rstride) {
      const unsigned wo = (unsigned)p % (unsigned)Wo;
      const unsigned t = (unsigned)p / (unsigned)Wo;
      const int ho = (int)(t % (unsigned)Ho);
      const int n = (int)(t / (unsigned)Ho);
      const int hb = ho * STRIDE - pad, wb = (int)wo * STRIDE - pad;
      bf16x8 vdy;
      vdy.v = *reinterpret_cast<const uint4*>(dy + (long)p * C + (long)vec * 8);
      bf16x8 vx[DW_K * DW_K];
      #pragma unroll
      for (int r = 0; r < DW_K; ++r) {
        const int h = hb + r;
        const bool okr = (h >= 0) && (h < H);
        const int hc = clamp_tap(h, H - 1);
        #pragma unroll
        for (int s = 0; s < DW_K; ++s) {
          const int w = wb + s;
          const bool ok = okr && (w >= 0) && (w < W_);
          const int wc = clamp_tap(w, W_ - 1);
          vx[r * DW_K + s].v = *reinterpret_cast<const uint4*>(
              x + (long)((n * H + hc) * W_ + wc) * C + (long)vec * 8);
          if (!ok) vx[r * DW_K + s].v = make_uint4(0u, 0u, 0u, 0u);
        }
      }
      float g[8];
      #pragma unroll
      for (int k = 0; k < 8; ++k) g[k] = b2f(vdy.h[k]);
      #pragma unroll
      for (int t9 = 0; t9 < DW_K * DW_K; ++t9)
        #pragma unroll
        for (int k = 0; k < 8; ++k) acc[t9][k] += g[k] * b2f(vx[t9].h[k]);
    }
  }

  __shared__ float lds[256 * 8];
  float* pout = part + (long)blockIdx.y * (DW_K * DW_K) * C + (long)vec * 8;
  #pragma unroll
  for (int t = 0; t < DW_K * DW_K; ++t) {
    if (ROWG > 1) {                             // block-uniform
      rowgroup_reduce8(cg, lds, acc[t]);
      __syncthreads();                          // lds is reused by the next tap
    }
    if (active && rowg == 0) {
      float4* o = reinterpret_cast<float4*>(pout + (long)t * C);
      o[0] = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
      o[1] = make_float4(acc[t][4], acc[t][5], acc[t][6], acc[t][7]);
    }
  }
}

// sum the [nparts][9][C] partials in fixed order -> dw[C][9] fp32.
// Block = 32 channels x 8 part-groups of one tap (k_bn_grad_finalize's
// geometry: a one-thread-per-channel loop over the partials is pure load
// latency); group pg sums parts pg, pg+8, ... then group 0 adds the 8 group
// sums in order.
__global__ __launch_bounds__(256) void k_depthwise_wgrad_finalize(
    const float* __restrict__ part, float* __restrict__ dw, int C,
    int nparts) {
  const int cl = threadIdx.x & 31;
  const int pg = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const int t = blockIdx.y;                     // tap 0..8
  float a = 0.f;
  if (c < C)
    for (int p = pg; p < nparts; p += 8)
      a += part[((long)p * (DW_K * DW_K) + t) * C + c];
  __shared__ float la[8][32];
  la[pg][cl] = a;
  __syncthreads();
  if (pg == 0 && c < C) {
    #pragma unroll
    for (int g = 1; g < 8; ++g) a += la[g][cl];
    dw[(long)c * (DW_K * DW_K) + t] = a;
  }
}

// ---------------------------------------------------------------------------
// host entry points
// ---------------------------------------------------------------------------
static int dw_check(const char* who, int C, int R, int S, int stride, int pad,
                    int H, int W_, int Ho, int Wo) {
  const char* why = nullptr;
  if (C <= 0 || C % 8 != 0) why = "C must be a positive multiple of 8";
  else if (R != DW_K || S != DW_K) why = "kernel must be 3x3";
  else if (stride != 1 && stride != 2) why = "stride must be 1 or 2";
  else if (pad < 0) why = "pad must be >= 0";
  else if (H <= 0 || W_ <= 0 || Ho <= 0 || Wo <= 0) why = "empty spatial extent";
  else if (Ho != (H + 2 * pad - DW_K) / stride + 1 ||
           Wo != (W_ + 2 * pad - DW_K) / stride + 1)
    why = "output extent does not match input extent";
  return why ? ddlw_fail(who, why) : 0;
}

DDLW_EXPORT int ddlw_depthwise_fwd(const void* x, const void* w_t, void* y,
                                   int N, int H, int W_, int C, int Ho, int Wo,
                                   int R, int S, int stride, int pad,
                                   void* stream) {
  if (C % 8 != 0) return ddlw_fail("depthwise_fwd", "C must be a multiple of 8");
  long total = (long)N * Ho * Wo * (C >> 3);
  hipLaunchKernelGGL(k_depthwise_fwd, dim3(grid_1d(total)), dim3(256), 0,
                     (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)w_t,
                     (bf16_t*)y, N, H, W_, C, Ho, Wo, R, S, stride, pad);
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_depthwise_fwd_ep(const void* x, const void* w_t, void* y,
                                      const void* scale, const void* bias,
                                      int act, int N, int H, int W_, int C,
                                      int Ho, int Wo, int stride, int pad,
                                      void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("depthwise_fwd_ep", why); };
  if (C <= 0 || C % 8 != 0) return fail("C must be a positive multiple of 8");
  if (stride != 1 && stride != 2) return fail("stride must be 1 or 2");
  if (pad < 0) return fail("pad must be >= 0");
  if (act < 0 || act > 2) return fail("act must be 0, 1 or 2");
  if (!scale || !bias) return fail("scale and bias are required");
  if (N <= 0 || H <= 0 || W_ <= 0 || Ho <= 0 || Wo <= 0)
    return fail("empty extent");
  if (Ho != (H + 2 * pad - 3) / stride + 1 || Wo != (W_ + 2 * pad - 3) / stride + 1)
    return fail("output extent does not match input extent");
  const long total = (long)N * Ho * Wo * (C >> 3);
  const int grid = grid_1d(total, 256, 4096);
  with_int<1, 2>(stride, [&](auto ST) {
    hipLaunchKernelGGL((k_depthwise_fwd_ep<decltype(ST)::value>), dim3(grid),
                       dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (const bf16_t*)w_t, (bf16_t*)y, (const float*)scale,
                       (const float*)bias, act, N, H, W_, C, Ho, Wo, pad);
  });
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_depthwise_dgrad(const void* dy, const void* w_t, void* dx,
                                     int N, int H, int W_, int C, int Ho,
                                     int Wo, int R, int S, int stride, int pad,
                                     void* stream) {
  if (int e = dw_check("depthwise_dgrad", C, R, S, stride, pad, H, W_, Ho, Wo))
    return e;
  const long total = (long)N * H * W_ * (C >> 3);
  if (total <= 0) return 0;
  with_int<1, 2>(stride, [&](auto ST) {
    hipLaunchKernelGGL((k_depthwise_dgrad<decltype(ST)::value>),
                       dim3(grid_1d(total)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)dy, (const bf16_t*)w_t, (bf16_t*)dx, N,
                       H, W_, C, Ho, Wo, pad);
  });
  DDLW_CHECK_LAUNCH();
}

// number of [9][C] row-slice partials the wgrad writes for `rows` = N*Ho*Wo
DDLW_EXPORT int ddlw_depthwise_wgrad_nparts(long rows, int C) {
  if (C < 8) return 1;
  return ColumnGeom(C).capped_slices(rows, DW_MAX_PARTS);
}

DDLW_EXPORT int ddlw_depthwise_wgrad(const void* dy, const void* x, void* part,
                                     void* dw, int N, int H, int W_, int C,
                                     int Ho, int Wo, int R, int S, int stride,
                                     int pad, void* stream) {
  if (int e = dw_check("depthwise_wgrad", C, R, S, stride, pad, H, W_, Ho, Wo))
    return e;
  if (N <= 0) return ddlw_fail("depthwise_wgrad", "empty batch");
  if ((long)N * H * W_ >= (1l << 30) || (long)N * Ho * Wo >= (1l << 30))
    return ddlw_fail("depthwise_wgrad",
                     "tensor too large for 32-bit pixel indexing");
  const int nparts = ddlw_depthwise_wgrad_nparts((long)N * Ho * Wo, C);
  dim3 grid(ColumnGeom(C).gx, nparts);
  with_int<1, 2>(stride, [&](auto ST) {
    hipLaunchKernelGGL((k_depthwise_wgrad_part<decltype(ST)::value>), grid,
                       dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy,
                       (const bf16_t*)x, (float*)part, N, H, W_, C, Ho, Wo,
                       pad);
  });
  hipLaunchKernelGGL(k_depthwise_wgrad_finalize,
                     dim3((C + 31) / 32, DW_K * DW_K), dim3(256), 0,
                     (hipStream_t)stream, (const float*)part, (float*)dw, C,
                     nparts);
  DDLW_CHECK_LAUNCH();
}
