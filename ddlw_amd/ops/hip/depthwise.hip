// Depthwise conv2d (K2 — MobileNetV2's depthwise blocks), NHWC bf16, fp32
// accumulation: training forward, eval forward with the folded-BN epilogue,
// the 3x3 backward (dgrad, wgrad + finalize), and the training stage fused
// with its BatchNorm (forward with statistics, stride-1 BN dx + dgrad + wgrad),
// and the backward of the stage under a FROZEN BatchNorm (stride 1 and 2).
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

// A loop-invariant bf16x8 vector stays packed (4 VGPRs) across a loop: without
// this the compiler hoists its bf16 -> fp32 unpacking out of the loop and the
// nine tap weight vectors cost 72 VGPRs instead of 36.
__device__ __forceinline__ void keep_packed(uint4& v) {
  asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
}

// The training kernels below are compiled without packed fp32 arithmetic
// (v_pk_fma_f32 and its kin), so every FMA of theirs is a plain VALU op on
// single registers: with the packed forms, which want aligned register pairs,
// the DX instances of k_depthwise_bwd_bn spill at 256 VGPRs.
// Side effect: a function of the runtime headers that is not always_inline
// (make_uint4, make_float4, __syncthreads) has other target features than
// these kernels and would stay an out-of-line CALL inside them, a full
// s_waitcnt in the tap loops. So they use none: dw_zero, dw_store4 and
// dw_barrier below inline, and the device assembly of both kernels is
// call-free (no s_swappc_b64).
#define DW_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))

typedef float dw_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void dw_zero(bf16x8& v) {
  v.v.x = 0u; v.v.y = 0u; v.v.z = 0u; v.v.w = 0u;
}

// The zeroing of an out-of-range tap as four ANDs with an all-ones / zero
// mask: written as `if (!ok) zero`, it is compiled to a divergent branch per
// tap, which ends the basic block, and every tap load then gets its own
// s_waitcnt vmcnt(0) instead of all nine being in flight.
__device__ __forceinline__ void dw_keep_if(bf16x8& v, bool ok) {
  const u32 m = ok ? 0xffffffffu : 0u;
  v.v.x &= m; v.v.y &= m; v.v.z &= m; v.v.w &= m;
}

__device__ __forceinline__ void dw_store4(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<dw_f32x4*>(p) = dw_f32x4{a, b, c, d};
}

// __syncthreads, spelled out
__device__ __forceinline__ void dw_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---------------------------------------------------------------------------
// Training forward with the BatchNorm statistics of its output, 3x3: the
// wgrad's column geometry instead of k_depthwise_fwd's grid-stride loop. A
// thread owns one 8-channel vector column, keeps the nine tap weight vectors
// in registers for the whole kernel and streams output pixels (neighbouring
// row groups sit on neighbouring pixels, so the tap re-reads hit cache). The
// statistics are the sums of the bf16-ROUNDED outputs and their squares (what
// k_bn_stats would read back), folded across row groups through LDS in fixed
// order; block (., y) owns partial row y. No atomics.
// ---------------------------------------------------------------------------
template <int STRIDE>
__global__ __launch_bounds__(256) DW_NO_PK_F32 void k_depthwise_fwd_stats(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w_t,
    bf16_t* __restrict__ y, float* __restrict__ psum, float* __restrict__ psq,
    int N, int H, int W_, int C, int Ho, int Wo, int pad) {
  const ColumnGeom cg(C);
  const int ROWG = cg.ROWG;
  const int vec = cg.vec(), rowg = cg.rowg();
  const bool active = cg.active();              // idle threads reach the barriers

  float s[8] = {0}, q[8] = {0};
  if (active) {
    bf16x8 vw[DW_K * DW_K];
    #pragma unroll
    for (int t = 0; t < DW_K * DW_K; ++t)
      vw[t].v = *reinterpret_cast<const uint4*>(w_t + (long)t * C + (long)vec * 8);
    // 32-bit pixel indexing, no unrolling across rows (k_depthwise_wgrad_part)
    const int rows = N * Ho * Wo;
    const int rstride = (int)gridDim.y * ROWG;
    #pragma unroll 1
    for (int p = (int)blockIdx.y * ROWG + rowg; p < rows; p += rstride) {
      const unsigned wo = (unsigned)p % (unsigned)Wo;
      const unsigned t = (unsigned)p / (unsigned)Wo;
      const int ho = (int)(t % (unsigned)Ho);
      const int n = (int)(t / (unsigned)Ho);
      const int hb = ho * STRIDE - pad, wb = (int)wo * STRIDE - pad;
      bf16x8 vx[DW_K * DW_K];
      #pragma unroll
      for (int r = 0; r < DW_K; ++r) {
        const int h = hb + r;
        const bool okr = (h >= 0) && (h < H);
        const int hc = clamp_tap(h, H - 1);
        #pragma unroll
        for (int c = 0; c < DW_K; ++c) {
          const int w = wb + c;
          const bool ok = okr && (w >= 0) && (w < W_);
          const int wc = clamp_tap(w, W_ - 1);
          vx[r * DW_K + c].v = *reinterpret_cast<const uint4*>(
              x + (long)((n * H + hc) * W_ + wc) * C + (long)vec * 8);
          dw_keep_if(vx[r * DW_K + c], ok);
        }
      }
      float acc[8] = {0};
      #pragma unroll
      for (int t9 = 0; t9 < DW_K * DW_K; ++t9) {
        keep_packed(vw[t9].v);
        #pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += b2f(vx[t9].h[k]) * b2f(vw[t9].h[k]);
      }
      bf16x8 o;
      #pragma unroll
      for (int k = 0; k < 8; ++k) {
        o.h[k] = f2b(acc[k]);
        const float f = b2f(o.h[k]);
        s[k] += f;
        q[k] += f * f;
      }
      *reinterpret_cast<uint4*>(y + (long)p * C + (long)vec * 8) = o.v;
    }
  }
  __shared__ float lds[256 * 8];
  if (ROWG > 1) {                               // block-uniform
    rowgroup_reduce8(cg, lds, s, dw_barrier);
    dw_barrier();
    rowgroup_reduce8(cg, lds, q, dw_barrier);
  }
  if (active && rowg == 0) {
    float* os = psum + (long)blockIdx.y * C + (long)vec * 8;
    float* oq = psq + (long)blockIdx.y * C + (long)vec * 8;
    dw_store4(os, s[0], s[1], s[2], s[3]);
    dw_store4(os + 4, s[4], s[5], s[6], s[7]);
    dw_store4(oq, q[0], q[1], q[2], q[3]);
    dw_store4(oq + 4, q[4], q[5], q[6], q[7]);
  }
}

// ---------------------------------------------------------------------------
// Stride-1 pad-1 backward of depthwise conv + BatchNorm in one kernel:
// k_bn_bwd_dx + k_depthwise_dgrad<1> + k_depthwise_wgrad_part<1> without the
// dz tensor between them. dz = A*g - B*y + D (g = dout under the mask, A, B,
// D per channel as k_bn_bwd_dx builds them) is recomputed where it is used.
//
// A block is DWB_TH x DWB_TW pixels x DWB_CV 8-channel vectors, one thread
// per (pixel, vector); the vector is tid % DWB_CV both when staging and when
// computing, so A, B, D and the nine weight vectors of the thread's channels
// live in registers. grid.x covers the channel groups, grid.y slices the
// list of (image, tile) pairs, and a block loops over its tiles:
//   1. stage dz of the tile plus a one-pixel halo into LDS, rounded to bf16
//      as the unfused route rounds it; positions outside the image are ZERO
//      (not D: no dz exists there). LDS is double-buffered, so one barrier
//      per tile is enough.
//   2. wgrad: dz of the own pixel (LDS) times x at the nine taps (global,
//      clamp_tap + zeroing), into 9 x 8 fp32 accumulators that live across
//      tiles;
//   3. dx (unless null): the nine neighbouring dz vectors from LDS times the
//      flipped taps. A tile pixel inside the image is written exactly once.
// At the end the accumulators are summed over the block's pixels through LDS
// in fixed order, one tap at a time, and the block writes ONE [9][C] partial
// in k_depthwise_wgrad_finalize's layout. No atomics.
// ---------------------------------------------------------------------------
#define DWB_TH 8
#define DWB_TW 8
#define DWB_CV 4
#define DWB_HW (DWB_TW + 2)                      // halo tile width
#define DWB_HALO ((DWB_TH + 2) * DWB_HW)         // halo tile pixels

template <int RELU, bool DX>
__global__ __launch_bounds__(256, 2) DW_NO_PK_F32 void k_depthwise_bwd_bn(
    const bf16_t* __restrict__ dout, const unsigned char* __restrict__ mask,
    const bf16_t* __restrict__ y, const bf16_t* __restrict__ x,
    const bf16_t* __restrict__ w_t, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ dbeta, const float* __restrict__ dgamma,
    bf16_t* __restrict__ dx, float* __restrict__ part, int N, int H, int W_,
    int C) {
  static_assert(DWB_TH * DWB_TW * DWB_CV == 256, "one thread per (pixel, vector)");
  const int vecC = C >> 3;
  const int tid = threadIdx.x;
  const int lv = tid % DWB_CV;                   // vector within the group
  const int lp = tid / DWB_CV;                   // pixel within the tile
  const int vec = blockIdx.x * DWB_CV + lv;
  const bool vok = vec < vecC;
  const long coff = (long)vec * 8;

  float A[8], B[8], D[8];
  bf16x8 vw[DW_K * DW_K];
  if (vok) {
    const float invM = 1.f / (float)((long)N * H * W_);
    #pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = vec * 8 + k;
      A[k] = gamma[c] * rstd[c];
      B[k] = A[k] * rstd[c] * dgamma[c] * invM;
      D[k] = B[k] * mean[c] - A[k] * dbeta[c] * invM;
    }
    if (DX) {
      #pragma unroll
      for (int t = 0; t < DW_K * DW_K; ++t)
        vw[t].v = *reinterpret_cast<const uint4*>(w_t + (long)t * C + coff);
    }
  }

  float acc[DW_K * DW_K][8];
  #pragma unroll
  for (int t = 0; t < DW_K * DW_K; ++t)
    #pragma unroll
    for (int k = 0; k < 8; ++k) acc[t][k] = 0.f;

  __shared__ uint4 sdz[2][DWB_HALO * DWB_CV];
  const int tiles_w = (W_ + DWB_TW - 1) / DWB_TW;
  const int tiles_h = (H + DWB_TH - 1) / DWB_TH;
  const int ntiles = N * tiles_h * tiles_w;
  const int py = lp / DWB_TW, px = lp % DWB_TW;
  int buf = 0;
  #pragma unroll 1
  for (int tile = (int)blockIdx.y; tile < ntiles; tile += (int)gridDim.y, buf ^= 1) {
    const unsigned tw = (unsigned)tile % (unsigned)tiles_w;
    const unsigned tt = (unsigned)tile / (unsigned)tiles_w;
    const int th = (int)(tt % (unsigned)tiles_h);
    const int n = (int)(tt / (unsigned)tiles_h);
    const int h0 = th * DWB_TH, w0 = (int)tw * DWB_TW;

    // 1. dz of the tile + halo -> LDS (item = halo pixel * DWB_CV + lv)
    #pragma unroll 1
    for (int it = tid; it < DWB_HALO * DWB_CV; it += 256) {
      const int hp = it / DWB_CV;
      const int h = h0 - 1 + hp / DWB_HW, w = w0 - 1 + hp % DWB_HW;
      bf16x8 o;
      dw_zero(o);
      if (vok && h >= 0 && h < H && w >= 0 && w < W_) {
        const int pix = (n * H + h) * W_ + w;
        bf16x8 vg, vy;
        vg.v = *reinterpret_cast<const uint4*>(dout + (long)pix * C + coff);
        vy.v = *reinterpret_cast<const uint4*>(y + (long)pix * C + coff);
        const unsigned mb = RELU ? mask[(long)pix * vecC + vec] : 0xffu;
        #pragma unroll
        for (int k = 0; k < 8; ++k) {
          float g = b2f(vg.h[k]);
          if (RELU && !((mb >> k) & 1)) g = 0.f;
          o.h[k] = f2b(A[k] * g - B[k] * b2f(vy.h[k]) + D[k]);
        }
      }
      sdz[buf][it] = o.v;
    }
    dw_barrier();

    const int h = h0 + py, w = w0 + px;
    if (vok && h < H && w < W_) {
      // 2. wgrad, one tap row of x in flight at a time
      bf16x8 own;
      own.v = sdz[buf][((py + 1) * DWB_HW + px + 1) * DWB_CV + lv];
      float g[8];
      #pragma unroll
      for (int k = 0; k < 8; ++k) g[k] = b2f(own.h[k]);
      #pragma unroll
      for (int r = 0; r < DW_K; ++r) {
        const int hh = h - 1 + r;
        const bool okr = (hh >= 0) && (hh < H);
        const int hc = clamp_tap(hh, H - 1);
        bf16x8 vx[DW_K];
        #pragma unroll
        for (int c = 0; c < DW_K; ++c) {
          const int ww = w - 1 + c;
          const bool ok = okr && (ww >= 0) && (ww < W_);
          const int wc = clamp_tap(ww, W_ - 1);
          vx[c].v = *reinterpret_cast<const uint4*>(
              x + (long)((n * H + hc) * W_ + wc) * C + coff);
          dw_keep_if(vx[c], ok);
        }
        #pragma unroll
        for (int c = 0; c < DW_K; ++c)
          #pragma unroll
          for (int k = 0; k < 8; ++k)
            acc[r * DW_K + c][k] += g[k] * b2f(vx[c].h[k]);
        // the next row's loads stay behind this row's FMAs: all nine taps
        // in flight at once spill
        asm volatile("" ::: "memory");
      }
      // 3. dx[h][w] = sum_{r,c} dz[h + 1 - r][w + 1 - c] * w[r][c]
      if (DX) {
        float a[8] = {0};
        #pragma unroll
        for (int r = 0; r < DW_K; ++r)
          #pragma unroll
          for (int c = 0; c < DW_K; ++c) {
            keep_packed(vw[r * DW_K + c].v);
            bf16x8 vd;
            vd.v = sdz[buf][((py + 2 - r) * DWB_HW + px + 2 - c) * DWB_CV + lv];
            #pragma unroll
            for (int k = 0; k < 8; ++k)
              a[k] += b2f(vd.h[k]) * b2f(vw[r * DW_K + c].h[k]);
          }
        bf16x8 o;
        #pragma unroll
        for (int k = 0; k < 8; ++k) o.h[k] = f2b(a[k]);
        *reinterpret_cast<uint4*>(dx + (long)((n * H + h) * W_ + w) * C + coff) = o.v;
      }
    }
  }

  // fold the accumulators over the block's 64 pixels, one tap at a time:
  // thread (grp, out) sums pixels grp*8 .. grp*8+7 of output out = (lv, k)
  // in order, then the first 32 threads add the 8 group sums in order
  __shared__ float red[256 * 8];
  __shared__ float red2[8][DWB_CV * 8];
  const int out = tid % (DWB_CV * 8), grp = tid / (DWB_CV * 8);
  const int ov = out >> 3, ok8 = out & 7;
  const int ovec = blockIdx.x * DWB_CV + ov;
  float* pout = part + (long)blockIdx.y * (DW_K * DW_K) * C + (long)ovec * 8 + ok8;
  #pragma unroll
  for (int t = 0; t < DW_K * DW_K; ++t) {
    #pragma unroll
    for (int k = 0; k < 8; ++k) red[tid * 8 + k] = acc[t][k];
    dw_barrier();
    float a = 0.f;
    #pragma unroll
    for (int i = 0; i < 8; ++i) a += red[((grp * 8 + i) * DWB_CV + ov) * 8 + ok8];
    red2[grp][out] = a;
    dw_barrier();                            // also frees red for the next tap
    if (grp == 0 && ovec < vecC) {
      a = red2[0][out];
      #pragma unroll
      for (int i = 1; i < 8; ++i) a += red2[i][out];
      pout[(long)t * C] = a;
    }
  }
}

// ---------------------------------------------------------------------------
// Pad-1 backward of depthwise conv + FROZEN BatchNorm (+ ReLU6), stride 1 or
// 2, in one kernel. With constant statistics dz needs no reduction:
//   g16 = gate(out) ? bf16(fp32(dout) * scale[c]) : 0,
//   gate = 1 (ACT 0) | 0 < out < 6 on the saved bf16 output (ACT 2),
// the definition of pointwise_frozen.hip, formed while staging.
//
// k_depthwise_bwd_bn's persistent design (8 x 8 pixels x DWB_CV vectors per
// block, grid.y slices the (image, tile) list, g16 of the tile plus halo
// double-buffered in LDS as bf16, wgrad accumulators in registers across
// tiles, one [9][C] partial per block for k_depthwise_wgrad_finalize), with
// the tile laid over the INPUT pixels, which is what lets stride 2 in: input
// pixel (h, w) meets output pixel ((h+1-r)/S, (w+1-s)/S) through tap (r, s)
// when both divisions are exact, and that one g16 vector serves both
//   dx[h][w]  += g16 * w[r][s]     and     dW[r][s] += g16 * x[h][w].
// So a thread loads its own x vector once (no tap loads from global, clamped
// or otherwise), reads nine g16 vectors from LDS and feeds both sums. The
// staged g16 tile is 10 x 10 output pixels from (h0-1, w0-1) at stride 1 and
// 5 x 5 from (h0/2, w0/2) at stride 2 (h0, w0 multiples of 8); positions
// outside the output are ZERO, and at stride 2 a tap of the wrong parity
// reads an in-range slot and is masked. No atomics, fixed order.
// ---------------------------------------------------------------------------
template <int STRIDE, int ACT, bool DX>
__global__ __launch_bounds__(256, 2) DW_NO_PK_F32 void k_depthwise_bwd_gated(
    const bf16_t* __restrict__ dout, const bf16_t* __restrict__ out,
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w_t,
    const float* __restrict__ scale, bf16_t* __restrict__ dx,
    float* __restrict__ part, int N, int H, int W_, int C, int Ho, int Wo) {
  static_assert(DWB_TH * DWB_TW * DWB_CV == 256, "one thread per (pixel, vector)");
  static_assert(DWB_TH == 8 && DWB_TW == 8, "tile origins must be even");
  constexpr int GW = STRIDE == 1 ? DWB_TW + 2 : DWB_TW / 2 + 1;   // staged width
  constexpr int GH = STRIDE == 1 ? DWB_TH + 2 : DWB_TH / 2 + 1;
  const int vecC = C >> 3;
  const int tid = threadIdx.x;
  const int lv = tid % DWB_CV;                   // vector within the group
  const int lp = tid / DWB_CV;                   // pixel within the tile
  const int vec = blockIdx.x * DWB_CV + lv;
  const bool vok = vec < vecC;
  const long coff = (long)vec * 8;

  float sc[8];
  bf16x8 vw[DW_K * DW_K];
  if (vok) {
    #pragma unroll
    for (int k = 0; k < 8; ++k) sc[k] = scale[vec * 8 + k];
    if (DX) {
      #pragma unroll
      for (int t = 0; t < DW_K * DW_K; ++t)
        vw[t].v = *reinterpret_cast<const uint4*>(w_t + (long)t * C + coff);
    }
  }

  float acc[DW_K * DW_K][8];
  #pragma unroll
  for (int t = 0; t < DW_K * DW_K; ++t)
    #pragma unroll
    for (int k = 0; k < 8; ++k) acc[t][k] = 0.f;

  __shared__ uint4 sg[2][GH * GW * DWB_CV];
  const int tiles_w = (W_ + DWB_TW - 1) / DWB_TW;
  const int tiles_h = (H + DWB_TH - 1) / DWB_TH;
  const int ntiles = N * tiles_h * tiles_w;
  const int py = lp / DWB_TW, px = lp % DWB_TW;
  int buf = 0;
  #pragma unroll 1
  for (int tile = (int)blockIdx.y; tile < ntiles; tile += (int)gridDim.y, buf ^= 1) {
    const unsigned tw = (unsigned)tile % (unsigned)tiles_w;
    const unsigned tt = (unsigned)tile / (unsigned)tiles_w;
    const int th = (int)(tt % (unsigned)tiles_h);
    const int n = (int)(tt / (unsigned)tiles_h);
    const int h0 = th * DWB_TH, w0 = (int)tw * DWB_TW;
    const int gh0 = STRIDE == 1 ? h0 - 1 : h0 / 2;
    const int gw0 = STRIDE == 1 ? w0 - 1 : w0 / 2;

    // 1. g16 of the staged output pixels -> LDS (item = pixel * DWB_CV + lv)
    #pragma unroll 1
    for (int it = tid; it < GH * GW * DWB_CV; it += 256) {
      const int gp = it / DWB_CV;
      const int ho = gh0 + gp / GW, wo = gw0 + gp % GW;
      bf16x8 o;
      dw_zero(o);
      if (vok && ho >= 0 && ho < Ho && wo >= 0 && wo < Wo) {
        const int pix = (n * Ho + ho) * Wo + wo;
        bf16x8 vg, vy;
        vg.v = *reinterpret_cast<const uint4*>(dout + (long)pix * C + coff);
        if (ACT == 2) vy.v = *reinterpret_cast<const uint4*>(out + (long)pix * C + coff);
        #pragma unroll
        for (int k = 0; k < 8; ++k) {
          o.h[k] = f2b(b2f(vg.h[k]) * sc[k]);
          if (ACT == 2) {
            const float ov = b2f(vy.h[k]);
            if (!(ov > 0.f && ov < 6.f)) o.h[k] = 0;
          }
        }
      }
      sg[buf][it] = o.v;
    }
    dw_barrier();

    const int h = h0 + py, w = w0 + px;
    if (vok && h < H && w < W_) {
      bf16x8 own;
      own.v = *reinterpret_cast<const uint4*>(x + (long)((n * H + h) * W_ + w) * C + coff);
      float xf[8], a[8];
      #pragma unroll
      for (int k = 0; k < 8; ++k) { xf[k] = b2f(own.h[k]); a[k] = 0.f; }
      // 2. tap (r, s): output pixel ((h+1-r)/S, (w+1-s)/S). In tile terms
      // q = py + 1 - r in [-1, 8]: slot q + 1 at stride 1; at stride 2 slot
      // q / 2 when q is even, and (q + 1) >> 1 is that slot for an even q
      // and an in-range one (masked) for an odd q.
      #pragma unroll
      for (int r = 0; r < DW_K; ++r) {
        const int qy = py + 1 - r;
        const int ly = STRIDE == 1 ? qy + 1 : (qy + 1) >> 1;
        const bool oky = STRIDE == 1 || !(qy & 1);
        #pragma unroll
        for (int s = 0; s < DW_K; ++s) {
          const int qx = px + 1 - s;
          const int lx = STRIDE == 1 ? qx + 1 : (qx + 1) >> 1;
          const bool ok = oky && (STRIDE == 1 || !(qx & 1));
          bf16x8 vd;
          vd.v = sg[buf][(ly * GW + lx) * DWB_CV + lv];
          if (STRIDE != 1) dw_keep_if(vd, ok);
          float g[8];
          #pragma unroll
          for (int k = 0; k < 8; ++k) {
            g[k] = b2f(vd.h[k]);
            acc[r * DW_K + s][k] += g[k] * xf[k];
          }
          if (DX) {
            keep_packed(vw[r * DW_K + s].v);
            #pragma unroll
            for (int k = 0; k < 8; ++k) a[k] += g[k] * b2f(vw[r * DW_K + s].h[k]);
          }
        }
      }
      if (DX) {
        bf16x8 o;
        #pragma unroll
        for (int k = 0; k < 8; ++k) o.h[k] = f2b(a[k]);
        *reinterpret_cast<uint4*>(dx + (long)((n * H + h) * W_ + w) * C + coff) = o.v;
      }
    }
  }

  // fold the accumulators over the block's 64 pixels, one tap at a time, as
  // k_depthwise_bwd_bn does: thread (grp, out) sums pixels grp*8 .. grp*8+7
  // of output out = (lv, k) in order, then the first 32 threads add the 8
  // group sums in order
  __shared__ float red[256 * 8];
  __shared__ float red2[8][DWB_CV * 8];
  const int outi = tid % (DWB_CV * 8), grp = tid / (DWB_CV * 8);
  const int ov = outi >> 3, ok8 = outi & 7;
  const int ovec = blockIdx.x * DWB_CV + ov;
  float* pout = part + (long)blockIdx.y * (DW_K * DW_K) * C + (long)ovec * 8 + ok8;
  #pragma unroll
  for (int t = 0; t < DW_K * DW_K; ++t) {
    #pragma unroll
    for (int k = 0; k < 8; ++k) red[tid * 8 + k] = acc[t][k];
    dw_barrier();
    float a = 0.f;
    #pragma unroll
    for (int i = 0; i < 8; ++i) a += red[((grp * 8 + i) * DWB_CV + ov) * 8 + ok8];
    red2[grp][outi] = a;
    dw_barrier();                            // also frees red for the next tap
    if (grp == 0 && ovec < vecC) {
      a = red2[0][outi];
      #pragma unroll
      for (int i = 1; i < 8; ++i) a += red2[i][outi];
      pout[(long)t * C] = a;
    }
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

// number of [C] statistics partial rows the training forward writes for
// `rows` = N*Ho*Wo (<= DW_MAX_PARTS: they go straight into k_bn_finalize);
// launches nothing, `stream` is unused (as in ddlw_pw_conv_nparts)
DDLW_EXPORT int ddlw_depthwise_fwd_stats_nparts(long rows, int C, void* stream) {
  (void)stream;
  if (C < 8) return 1;
  return ColumnGeom(C).capped_slices(rows, DW_MAX_PARTS);
}

DDLW_EXPORT int ddlw_depthwise_fwd_stats(const void* x, const void* w_t, void* y,
                                         void* psum, void* psq, int N, int H,
                                         int W_, int C, int Ho, int Wo,
                                         int stride, int pad, void* stream) {
  if (int e = dw_check("depthwise_fwd_stats", C, DW_K, DW_K, stride, pad, H, W_,
                       Ho, Wo))
    return e;
  if (N <= 0) return ddlw_fail("depthwise_fwd_stats", "empty batch");
  if ((long)N * H * W_ >= (1l << 30) || (long)N * Ho * Wo >= (1l << 30))
    return ddlw_fail("depthwise_fwd_stats",
                     "tensor too large for 32-bit pixel indexing");
  const int nparts = ddlw_depthwise_fwd_stats_nparts((long)N * Ho * Wo, C, nullptr);
  dim3 grid(ColumnGeom(C).gx, nparts);
  with_int<1, 2>(stride, [&](auto ST) {
    hipLaunchKernelGGL((k_depthwise_fwd_stats<decltype(ST)::value>), grid,
                       dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (const bf16_t*)w_t, (bf16_t*)y, (float*)psum,
                       (float*)psq, N, H, W_, C, Ho, Wo, pad);
  });
  DDLW_CHECK_LAUNCH();
}

// number of [9][C] partials of the fused backward: one per persistent block
// row, at most one per (image, tile) pair
DDLW_EXPORT int ddlw_depthwise_bwd_bn_nparts(int N, int H, int W_, void* stream) {
  (void)stream;
  const long tiles = (long)N * cdiv(H, DWB_TH) * cdiv(W_, DWB_TW);
  return (int)(tiles < DW_MAX_PARTS ? (tiles > 0 ? tiles : 1) : DW_MAX_PARTS);
}

// dx may be null (no input gradient wanted). part: [nparts][9][C] fp32
// scratch, dw: [C][9] fp32.
DDLW_EXPORT int ddlw_depthwise_bwd_bn(const void* dout, const void* mask,
                                      const void* y, const void* x,
                                      const void* w_t, const void* mean,
                                      const void* rstd, const void* gamma,
                                      const void* dbeta, const void* dgamma,
                                      void* dx, void* part, void* dw, int N,
                                      int H, int W_, int C, int relu,
                                      void* stream) {
  if (int e = dw_check("depthwise_bwd_bn", C, DW_K, DW_K, 1, 1, H, W_, H, W_))
    return e;
  if (N <= 0) return ddlw_fail("depthwise_bwd_bn", "empty batch");
  if (relu && !mask) return ddlw_fail("depthwise_bwd_bn", "relu needs the mask");
  if ((long)N * H * W_ >= (1l << 30))
    return ddlw_fail("depthwise_bwd_bn",
                     "tensor too large for 32-bit pixel indexing");
  const int nparts = ddlw_depthwise_bwd_bn_nparts(N, H, W_, nullptr);
  dim3 grid((unsigned)cdiv(C >> 3, DWB_CV), nparts);
  with_int<0, 1>(relu, [&](auto RELU) {
    with_bool(dx != nullptr, [&](auto DX) {
      hipLaunchKernelGGL(
          (k_depthwise_bwd_bn<decltype(RELU)::value, decltype(DX)::value>),
          grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dout,
          (const unsigned char*)mask, (const bf16_t*)y, (const bf16_t*)x,
          (const bf16_t*)w_t, (const float*)mean, (const float*)rstd,
          (const float*)gamma, (const float*)dbeta, (const float*)dgamma,
          (bf16_t*)dx, (float*)part, N, H, W_, C);
    });
  });
  hipLaunchKernelGGL(k_depthwise_wgrad_finalize,
                     dim3((C + 31) / 32, DW_K * DW_K), dim3(256), 0,
                     (hipStream_t)stream, (const float*)part, (float*)dw, C,
                     nparts);
  DDLW_CHECK_LAUNCH();
}

// Frozen-BN backward, 3x3 pad 1, stride 1 or 2. dout/out [N][Ho][Wo][C], x
// and dx [N][H][W][C] bf16; dx may be null (no input gradient wanted); out is
// read under act 2 (ReLU6) only. part: [ddlw_depthwise_bwd_bn_nparts(N, H,
// W)][9][C] fp32 scratch (the tiles lie over the input), dw: [C][9] fp32.
DDLW_EXPORT int ddlw_depthwise_bwd_gated(const void* dout, const void* out,
                                         const void* x, const void* w_t,
                                         const void* scale, void* dx,
                                         void* part, void* dw, int N, int H,
                                         int W_, int C, int Ho, int Wo,
                                         int stride, int act, void* stream) {
  if (int e = dw_check("depthwise_bwd_gated", C, DW_K, DW_K, stride, 1, H, W_,
                       Ho, Wo))
    return e;
  auto fail = [](const char* why) { return ddlw_fail("depthwise_bwd_gated", why); };
  if (N <= 0) return fail("empty batch");
  if (act != 0 && act != 2) return fail("act must be 0 (none) or 2 (ReLU6)");
  if (!dout || !x || !scale || !part || !dw || (act == 2 && !out) || (dx && !w_t))
    return fail("dout, x, scale, part, dw (out under ReLU6, w_t with dx) are required");
  if ((long)N * H * W_ >= (1l << 30))
    return fail("tensor too large for 32-bit pixel indexing");
  const int nparts = ddlw_depthwise_bwd_bn_nparts(N, H, W_, nullptr);
  dim3 grid((unsigned)cdiv(C >> 3, DWB_CV), nparts);
  with_int<1, 2>(stride, [&](auto ST) {
    with_int<0, 2>(act, [&](auto ACTc) {
      with_bool(dx != nullptr, [&](auto DX) {
        hipLaunchKernelGGL(
            (k_depthwise_bwd_gated<decltype(ST)::value, decltype(ACTc)::value,
                                   decltype(DX)::value>),
            grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dout,
            (const bf16_t*)out, (const bf16_t*)x, (const bf16_t*)w_t,
            (const float*)scale, (bf16_t*)dx, (float*)part, N, H, W_, C, Ho, Wo);
      });
    });
  });
  DDLW_CHECK_LAUNCH_OR_RETURN();
  hipLaunchKernelGGL(k_depthwise_wgrad_finalize,
                     dim3((C + 31) / 32, DW_K * DW_K), dim3(256), 0,
                     (hipStream_t)stream, (const float*)part, (float*)dw, C,
                     nparts);
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
