// Frozen-MobileNetV2 pointwise (1x1, stride 1, pad 0) conv on MFMA with the
// folded-BN epilogue (k_depthwise_fwd_ep in depthwise.hip applies the same one)
//   y = act(conv(x) * scale[k] + bias[k] (+ res)),   act: 0 none, 1 ReLU, 2 ReLU6
// NHWC bf16 in/out, fp32 accumulation and epilogue, one rounding to bf16.
// The fine-tuned suffix trains on the same GEMM: k_pw_conv_stats is the
// forward with the BatchNorm statistics in its epilogue, and dgrad is
// k_pw_conv on (dy, w^T) with the accumulate tensor as the residual.
//
// k_pw_conv — y[m][k] = sum_c x[m][c] * w[k][c], a plain GEMM over NHWC rows.
// These layers are small-C, short-K-loop and HBM-bound, so the kernel is
// built around its global traffic, not around MFMA rate:
//   - v_mfma_f32_16x16x32_bf16 with W as the A operand and x as the B
//     operand (D = W_tile * x_tile^T). Both fragments are "8 consecutive
//     channels of one row" = one 16-byte global load per lane, so nothing is
//     staged through LDS and the kernel has no barrier: x and y stream
//     through once, W (<= 800 KB) is served from L1/L2.
//   - tails by predicated register staging: a lane whose 8-channel vector
//     lies past C (or whose row lies past M / K) loads from a clamped,
//     in-bounds address of its own row and is then zeroed, so the tail of
//     the last 32-deep step contributes exactly zero and no neighbouring
//     row's bytes are ever multiplied.
//   - D puts the m index on lane&15 and 4 output channels in the 4
//     accumulator registers. The two W fragments of a pair take their rows
//     in the order k = 8*(i>>2) + 4*f + (i&3), so a lane ends up with 8
//     CONSECUTIVE output channels of one row: scale/bias come in as two
//     float4, the residual as one 16-byte load, y leaves as one 16-byte
//     store (16 rows x 64 B per wave instruction). K % 8 == 0 makes every
//     such vector wholly inside or wholly outside K.
//   - a wave owns 32 rows x 32*NP output channels (NP = 1,2,3,5,6 covers the
//     MobileNetV2 K values with little waste), a block 4 waves = 128 rows.
//     Consecutive blocks walk the N tiles of one row tile so the re-read of
//     x comes from cache.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 pw_bf16x8;
typedef __attribute__((ext_vector_type(4))) float pw_f32x4;

#define PW_MR 2                    // 16-row fragments per wave
#define PW_WAVES 4
#define PW_BM (PW_WAVES * PW_MR * 16)

// The tile/MFMA body, shared AS TEXT by k_pw_conv and k_pw_conv_stats. (As an
// inlined device function the same statements change the emitted code of the
// frozen-path k_pw_conv instantiations — bench/tools/device_asm.py; as a macro
// they cannot.) Reads x, w, M, C, K, m0, k0, l15, lg and NP of the enclosing
// kernel and leaves acc[p][f][mi]: the wave's 32 rows from m0 x 32*NP output
// channels from k0. Row pointers are clamped in bounds with validity kept
// aside; a row past M, a weight row past K and a channel vector past C
// (C % 8 == 0: whole vectors) are loaded from the clamped address and zeroed,
// so their accumulators are exactly zero.
#define PW_TILE_MMA()                                                                      \
    const bf16_t* xrow[PW_MR];                                                           \
    bool xok[PW_MR];                                                                     \
    _Pragma("unroll")                                                                    \
    for (int mi = 0; mi < PW_MR; ++mi) {                                                 \
      const long m = m0 + mi * 16 + l15;                                                 \
      xok[mi] = m < M;                                                                   \
      xrow[mi] = x + (xok[mi] ? m : M - 1) * C;                                          \
    }                                                                                    \
    const bf16_t* wrow[NP][2];                                                           \
    bool wok[NP][2];                                                                     \
    _Pragma("unroll")                                                                    \
    for (int p = 0; p < NP; ++p)                                                         \
      _Pragma("unroll")                                                                  \
      for (int f = 0; f < 2; ++f) {                                                      \
        const int k = k0 + p * 32 + (l15 >> 2) * 8 + f * 4 + (l15 & 3);                  \
        wok[p][f] = k < K;                                                               \
        wrow[p][f] = w + (long)(wok[p][f] ? k : K - 1) * C;                              \
      }                                                                                  \
                                                                                         \
    pw_f32x4 acc[NP][2][PW_MR];                                                          \
    _Pragma("unroll")                                                                    \
    for (int p = 0; p < NP; ++p)                                                         \
      _Pragma("unroll")                                                                  \
      for (int f = 0; f < 2; ++f)                                                        \
        _Pragma("unroll")                                                                \
        for (int mi = 0; mi < PW_MR; ++mi) acc[p][f][mi] = pw_f32x4{0.f, 0.f, 0.f, 0.f}; \
                                                                                         \
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);                                       \
    for (int c0 = 0; c0 < C; c0 += 32) {                                                 \
      const int c = c0 + lg * 8;                                                         \
      const bool cok = c < C;                                                            \
      const int cc = cok ? c : 0;                                                        \
      union { uint4 u; pw_bf16x8 v; } fx[PW_MR], fw[NP][2];                              \
      _Pragma("unroll")                                                                  \
      for (int mi = 0; mi < PW_MR; ++mi) {                                               \
        fx[mi].u = *reinterpret_cast<const uint4*>(xrow[mi] + cc);                       \
        if (!(cok && xok[mi])) fx[mi].u = zero;                                          \
      }                                                                                  \
      _Pragma("unroll")                                                                  \
      for (int p = 0; p < NP; ++p)                                                       \
        _Pragma("unroll")                                                                \
        for (int f = 0; f < 2; ++f) {                                                    \
          fw[p][f].u = *reinterpret_cast<const uint4*>(wrow[p][f] + cc);                 \
          if (!(cok && wok[p][f])) fw[p][f].u = zero;                                    \
        }                                                                                \
      _Pragma("unroll")                                                                  \
      for (int p = 0; p < NP; ++p)                                                       \
        _Pragma("unroll")                                                                \
        for (int f = 0; f < 2; ++f)                                                      \
          _Pragma("unroll")                                                              \
          for (int mi = 0; mi < PW_MR; ++mi)                                             \
            acc[p][f][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                     \
                fw[p][f].v, fx[mi].v, acc[p][f][mi], 0, 0, 0);                           \
    }

template <int NP, bool HAS_RES>
__global__ __launch_bounds__(256) void k_pw_conv(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ y, const bf16_t* __restrict__ res,
    const float* __restrict__ scale, const float* __restrict__ bias, int act,
    long M, int C, int K, int ntiles) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long mtile = blockIdx.x / ntiles;
  const int ntile = blockIdx.x - (int)(mtile * ntiles);
  const int l15 = lane & 15;
  const int lg = lane >> 4;                      // 0..3: channel group of 8
  const long m0 = mtile * PW_BM + wave * (PW_MR * 16);
  const int k0 = ntile * (NP * 32);

  PW_TILE_MMA();

  // epilogue: lane (lg, l15) holds channels kb .. kb+7 of row m0 + mi*16 + l15
  #pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int kb = k0 + p * 32 + lg * 8;
    if (kb >= K) continue;
    float sc[8], bi[8];
    if (scale) {
      load8f(scale + kb, sc);
      load8f(bias + kb, bi);
    } else {
      #pragma unroll
      for (int e = 0; e < 8; ++e) { sc[e] = 1.f; bi[e] = 0.f; }
    }
    #pragma unroll
    for (int mi = 0; mi < PW_MR; ++mi) {
      const long m = m0 + mi * 16 + l15;
      if (m >= M) continue;
      const long oi = m * K + kb;
      float v[8];
      #pragma unroll
      for (int e = 0; e < 8; ++e)
        v[e] = acc[p][e >> 2][mi][e & 3] * sc[e] + bi[e];
      if constexpr (HAS_RES) {
        bf16x8 r;
        r.v = *reinterpret_cast<const uint4*>(res + oi);
        #pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += b2f(r.h[e]);
      }
      bf16x8 o;
      #pragma unroll
      for (int e = 0; e < 8; ++e) o.h[e] = f2b(apply_act(v[e], act));
      *reinterpret_cast<uint4*>(y + oi) = o.v;
    }
  }
}

// k_pw_conv_stats — the training forward: y = x * w^T with no epilogue math,
// plus the BatchNorm statistics of y as per-block partial rows
//   psum[mtile][k] = sum over the block's 128 rows of y[m][k],  psq: of y^2
// ([cdiv(M,128)][K] fp32, consumed by k_bn_finalize / k_bn_parts_fold).
// The sums run over the bf16-ROUNDED outputs (the bn_partials_16 decision in
// conv_gemm.hip), so they are the statistics of the stored y. No atomics: a
// lane folds its 2 rows, a DPP row sum folds the 16 lanes, the 4 waves meet
// once in LDS after the (still barrier-free) main loop and are added in wave
// order; block (mtile, ntile) alone writes row mtile of its own N tile's
// channels. Rows past M and channels past K have zero accumulators
// (PW_TILE_MMA), so they add nothing and no sum is masked; only the stores
// are.
template <int NP>
__global__ __launch_bounds__(256) void k_pw_conv_stats(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ y, float* __restrict__ psum, float* __restrict__ psq,
    long M, int C, int K, int ntiles) {
  __shared__ __attribute__((aligned(16))) float red[2][PW_WAVES][NP * 32];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long mtile = blockIdx.x / ntiles;
  const int ntile = blockIdx.x - (int)(mtile * ntiles);
  const int l15 = lane & 15;
  const int lg = lane >> 4;
  const long m0 = mtile * PW_BM + wave * (PW_MR * 16);
  const int k0 = ntile * (NP * 32);

  PW_TILE_MMA();

  #pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int kb = k0 + p * 32 + lg * 8;
    float s[8], q[8];
    #pragma unroll
    for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
    #pragma unroll
    for (int mi = 0; mi < PW_MR; ++mi) {
      const long m = m0 + mi * 16 + l15;
      bf16x8 o;
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        o.h[e] = f2b(acc[p][e >> 2][mi][e & 3]);
        const float r = b2f(o.h[e]);
        s[e] += r;
        q[e] += r * r;
      }
      if (m < M && kb < K) *reinterpret_cast<uint4*>(y + m * K + kb) = o.v;
    }
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      s[e] = row_sum16(s[e]);
      q[e] = row_sum16(q[e]);
    }
    if (l15 == 0) {
      float* rs = &red[0][wave][p * 32 + lg * 8];
      float* rq = &red[1][wave][p * 32 + lg * 8];
      *reinterpret_cast<float4*>(rs) = make_float4(s[0], s[1], s[2], s[3]);
      *reinterpret_cast<float4*>(rs + 4) = make_float4(s[4], s[5], s[6], s[7]);
      *reinterpret_cast<float4*>(rq) = make_float4(q[0], q[1], q[2], q[3]);
      *reinterpret_cast<float4*>(rq + 4) = make_float4(q[4], q[5], q[6], q[7]);
    }
  }
  __syncthreads();
  const int t = threadIdx.x;                     // NP * 32 <= 192 < 256
  if (t < NP * 32 && k0 + t < K) {
    float ts = red[0][0][t], tq = red[1][0][t];
    #pragma unroll
    for (int wv = 1; wv < PW_WAVES; ++wv) {
      ts += red[0][wv][t];
      tq += red[1][wv][t];
    }
    psum[mtile * K + k0 + t] = ts;
    psq[mtile * K + k0 + t] = tq;
  }
}

// 32-channel fragment pairs per wave: the smallest listed NP that covers K in
// one tile, else whichever of 5 / 6 wastes fewer pairs over ceil(K/32).
static int pw_pick_np(int K) {
  const int kp = (K + 31) / 32;
  if (kp <= 3) return kp;
  if (kp <= 5) return 5;
  if (kp == 6) return 6;
  const int w5 = (kp + 4) / 5 * 5, w6 = (kp + 5) / 6 * 6;
  return w5 < w6 ? 5 : 6;
}

// x [M][C], w [K][C], y/res [M][K] bf16; scale/bias fp32 [K] (both or
// neither).
DDLW_EXPORT int ddlw_pw_conv_fwd(const void* x, const void* w, void* y,
                                 const void* res, const void* scale,
                                 const void* bias, int act, long M, int C,
                                 int K, void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("pw_conv_fwd", why); };
  if (C <= 0 || C % 8 != 0 || K <= 0 || K % 8 != 0)
    return fail("C and K must be positive multiples of 8");
  if (M < 0 || M >= (1l << 31)) return fail("M must be below 2^31");
  if (act < 0 || act > 2) return fail("act must be 0, 1 or 2");
  if ((scale == nullptr) != (bias == nullptr))
    return fail("scale and bias come together");
  if ((((size_t)x | (size_t)w | (size_t)y | (size_t)res | (size_t)scale |
        (size_t)bias) & 15) != 0)
    return fail("pointers must be 16-byte aligned");
  if (M == 0) return 0;
  const int np = pw_pick_np(K);
  const int ntiles = (K + np * 32 - 1) / (np * 32);
  const long blocks = cdiv(M, PW_BM) * ntiles;
  if (blocks >= (1l << 31)) return fail("grid too large");
  with_int<1, 2, 3, 5, 6>(np, [&](auto NPc) {
    with_bool(res != nullptr, [&](auto HR) {
      hipLaunchKernelGGL((k_pw_conv<decltype(NPc)::value, decltype(HR)::value>),
                         dim3((unsigned)blocks), dim3(256), 0,
                         (hipStream_t)stream, (const bf16_t*)x,
                         (const bf16_t*)w, (bf16_t*)y, (const bf16_t*)res,
                         (const float*)scale, (const float*)bias, act, M, C, K,
                         ntiles);
    });
  });
  DDLW_CHECK_LAUNCH();
}

// Partial rows ddlw_pw_conv_fwd_stats writes per channel: one per 128-row
// block; a channel's rows come from the blocks of its own N tile only, so the
// count does not depend on K. Launches nothing; `stream` is there because
// every export outside the ABI test's pinned query list ends in one.
DDLW_EXPORT int ddlw_pw_conv_nparts(long M, int K, void* stream) {
  (void)K;
  (void)stream;
  return (M < 0 || M >= (1l << 31)) ? -1 : (int)cdiv(M, PW_BM);
}

// Training forward: y = x * w^T (x [M][C], w [K][C], y [M][K] bf16) and the
// BN statistics partials of y, psum/psq fp32 [ddlw_pw_conv_nparts(M, K)][K].
DDLW_EXPORT int ddlw_pw_conv_fwd_stats(const void* x, const void* w, void* y,
                                       void* psum, void* psq, long M, int C,
                                       int K, void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("pw_conv_fwd_stats", why); };
  if (C <= 0 || C % 8 != 0 || K <= 0 || K % 8 != 0)
    return fail("C and K must be positive multiples of 8");
  if (M < 0 || M >= (1l << 31)) return fail("M must be below 2^31");
  if ((((size_t)x | (size_t)w | (size_t)y) & 15) != 0)
    return fail("x, w and y must be 16-byte aligned");
  if (psum == nullptr || psq == nullptr || (((size_t)psum | (size_t)psq) & 3) != 0)
    return fail("psum and psq must be fp32 buffers");
  if (M == 0) return 0;
  const int np = pw_pick_np(K);
  const int ntiles = (K + np * 32 - 1) / (np * 32);
  const long blocks = cdiv(M, PW_BM) * ntiles;
  if (blocks >= (1l << 31)) return fail("grid too large");
  with_int<1, 2, 3, 5, 6>(np, [&](auto NPc) {
    hipLaunchKernelGGL((k_pw_conv_stats<decltype(NPc)::value>),
                       dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)w,
                       (bf16_t*)y, (float*)psum, (float*)psq, M, C, K, ntiles);
  });
  DDLW_CHECK_LAUNCH();
}
