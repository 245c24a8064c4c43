// Frozen-MobileNetV2 tail: pointwise (1x1) conv + folded BN + activation +
// global average pool in one kernel. The K-channel map is never stored:
//   y[n,r,k] = bf16(act((sum_c x[n,r,c] * w[k,c]) * scale[k] + bias[k]))
//   p[n,k]   = bf16((sum_{r = 0 .. HW-1, in that order, fp32} y[n,r,k]) * (1.f / HW))
// x [N*HW][C] NHWC bf16, w [K][C] bf16, scale/bias fp32 [K] (both or
// neither), p [N][K] bf16. C % 8 == 0, 8 <= C <= 320, K % 8 == 0.
//
// The data contract is that of the two kernels it replaces, bit for bit:
// k_pw_conv (pointwise.hip) followed by k_gap_fwd (pool.hip). y is rounded to
// bf16 where k_pw_conv rounds it, the pool adds the rounded values in fp32 in
// row order from 0.f and multiplies by 1.f / HW as k_gap_fwd does. The MFMA
// operand placement and the reduction order are PW_TILE_MMA's
// (v_mfma_f32_16x16x32_bf16, W as A, x as B, 32-deep steps in ascending c,
// weight rows in the order k = 8*(i>>2) + 4*f + (i&3)), and the epilogue is
// the same expression, so the contraction is the same.
//
// Work split — the other way round from k_pw_conv, which gives a wave 32 rows
// and streams W past them:
//   - a workgroup of 4 waves owns 128 output channels (32 per wave: the two
//     16-row A fragments of one pair) and `imgs` consecutive images; the grid
//     is cdiv(K,128) x cdiv(N,imgs), the channel tiles of one image group on
//     consecutive blocks so x is re-read from cache;
//   - W in registers: a wave loads its 32 x C slab once (KS steps x 2
//     fragments x 4 VGPRs, 80 at C = 320; KS = 5 or 10 by C) and keeps it for
//     every image of the group. Steps past C, channel vectors past C and
//     weight rows past K are loaded from clamped addresses and zeroed;
//   - x through LDS: the 64-pixel tile of one image (contiguous in memory) is
//     staged once per workgroup, row stride 2*C + 16 bytes, and all four
//     waves read their B fragments from it. The tile of the NEXT unit (pixel
//     tile or image) is fetched into registers before the MFMAs of this one
//     and written to LDS after them: one x buffer, the global latency under
//     the MFMAs. Rows past HW are copies of the image's last row (a clamped,
//     in-bounds read): a pixel is a column of the MFMA and touches no other,
//     so they need no zeroing, they are only never summed;
//   - pool without cross-lane arithmetic: after the epilogue a lane holds 8
//     consecutive channels of one pixel, rounds them and stores them with one
//     16-byte LDS write into a 64 x 128 bounce tile (272-byte rows). Then one
//     thread per channel walks the valid rows in order and adds into its fp32
//     running sum, carried across pixel tiles: the sequential order of
//     k_gap_fwd, no atomics, DPP or shuffles, two calls bit-equal.
// LDS: 64 * (2*32*KS + 16) + 64 * 272 + 1024 (scale, bias) bytes = 60,416 at
// KS = 10.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 pwg_bf16x8;
typedef __attribute__((ext_vector_type(4))) float pwg_f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int pwg_u32x4;

#define PWG_BK 128                 // output channels per workgroup, 32 per wave
#define PWG_PT 64                  // pixels per tile
#define PWG_PF (PWG_PT / 16)       // MFMA column fragments per tile
#define PWG_YS (PWG_BK + 8)        // bounce row stride in bf16 (272 B)

// The staging walk of thread t: vector j of the thread is vector t + 256*j of
// the tile, row r = idx / vecC, vector v = idx % vecC, advanced without a
// division (256 = q*vecC + rem). 64 rows x vecC <= 64 * 4*KS vectors, so KS
// vectors per thread cover the tile.
struct PwgWalk {
  int r, v;
  __device__ __forceinline__ void next(int q, int rem, int vecC) {
    r += q;
    v += rem;
    if (v >= vecC) { v -= vecC; ++r; }
  }
};

// Issue the global loads of the 64-row tile from row tile0 of image n into
// registers. A row past HW reads the image's last row, and so does a vector
// of the walk that lies past the tile (never staged): every load is
// unconditional and in bounds, so pre[] stays in registers. Nothing here
// reads a loaded value, so the wave does not wait for them.
template <int KS>
__device__ __forceinline__ void pwg_fetch(pwg_u32x4 (&pre)[KS], const bf16_t* __restrict__ x,
                                          long n, int tile0, int HW, int C, int vecC,
                                          PwgWalk wk, int q, int rem) {
  const bf16_t* base = x + (n * HW + tile0) * C;
  const int last = HW - 1 - tile0;
  #pragma unroll
  for (int j = 0; j < KS; ++j) {
    const int rr = wk.r < last ? wk.r : last;    // also a walk past the tile: unused
    pre[j] = *reinterpret_cast<const pwg_u32x4*>(base + (long)rr * C + wk.v * 8);
    wk.next(q, rem, vecC);
  }
}

template <int KS>
__device__ __forceinline__ void pwg_stage(const pwg_u32x4 (&pre)[KS], bf16_t* xs, int xstride,
                                          int vecC, PwgWalk wk, int q, int rem) {
  #pragma unroll
  for (int j = 0; j < KS; ++j) {
    if (wk.r < PWG_PT)
      *reinterpret_cast<pwg_u32x4*>(xs + wk.r * xstride + wk.v * 8) = pre[j];
    wk.next(q, rem, vecC);
  }
}

template <int KS>
__global__ __launch_bounds__(256) void k_pw_conv_gap(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ p, const float* __restrict__ scale,
    const float* __restrict__ bias, int act, int N, int HW, int C, int K,
    int imgs, int ktiles) {
  __shared__ __attribute__((aligned(16))) bf16_t xs[PWG_PT * (KS * 32 + 8)];
  __shared__ __attribute__((aligned(16))) bf16_t ys[PWG_PT * PWG_YS];
  __shared__ __attribute__((aligned(16))) float sb[2 * PWG_BK];   // scale | bias
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int l15 = lane & 15;
  const int lg = lane >> 4;                      // 0..3: channel group of 8
  const int group = blockIdx.x / ktiles;
  const int ktile = blockIdx.x - group * ktiles;
  const int k0 = ktile * PWG_BK + wave * 32;
  const int n0 = group * imgs;
  const int nimg = (N - n0) < imgs ? (N - n0) : imgs;
  const int vecC = C >> 3;
  const int xstride = C + 8;
  const int steps = (C + 31) >> 5;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  // the wave's weight slab, held for every image of the group
  union { uint4 u; pwg_bf16x8 v; } wr[KS][2];
  #pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int k = k0 + (l15 >> 2) * 8 + f * 4 + (l15 & 3);
    const bool wok = k < K;
    const bf16_t* wrow = w + (long)(wok ? k : K - 1) * C;
    #pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int c = s * 32 + lg * 8;
      const bool cok = c < C;                    // C % 8 == 0: whole vectors
      wr[s][f].u = *reinterpret_cast<const uint4*>(wrow + (cok ? c : 0));
      if (!(cok && wok)) wr[s][f].u = zero;
    }
  }

  // folded BN of the workgroup's 128 channels, in LDS so that it holds no
  // registers across the MFMAs; visible after the first barrier of the loop
  {
    const int k = ktile * PWG_BK + (t & (PWG_BK - 1));
    const float* tab = t < PWG_BK ? scale : bias;
    sb[t] = (scale && k < K) ? tab[k] : (t < PWG_BK ? 1.f : 0.f);
  }

  const int q = 256 / vecC, rem = 256 - q * vecC;
  PwgWalk wk;
  wk.r = t / vecC;
  wk.v = t - wk.r * vecC;

  const float inv = 1.f / (float)HW;
  const int ptiles = (HW + PWG_PT - 1) / PWG_PT;
  const int units = nimg * ptiles;               // (image, pixel tile) pairs
  pwg_u32x4 pre[KS];
  pwg_fetch<KS>(pre, x, n0, 0, HW, C, vecC, wk, q, rem);
  int n = n0, tile0 = 0;
  float psum = 0.f;                              // thread t < 128: channel t
  for (int u = 0; u < units; ++u) {
    pwg_stage<KS>(pre, xs, xstride, vecC, wk, q, rem);
    __syncthreads();
    int nn = n, nt = tile0 + PWG_PT;
    if (nt >= HW) { nt = 0; ++nn; }
    if (u + 1 < units) pwg_fetch<KS>(pre, x, nn, nt, HW, C, vecC, wk, q, rem);

    pwg_f32x4 acc[2][PWG_PF];
    #pragma unroll
    for (int f = 0; f < 2; ++f)
      #pragma unroll
      for (int pf = 0; pf < PWG_PF; ++pf) acc[f][pf] = pwg_f32x4{0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (s < steps) {                           // uniform: a step past C adds exact zeros
        const int c = s * 32 + lg * 8;
        const bool cok = c < C;
        const int cc = cok ? c : 0;
        union { uint4 u; pwg_bf16x8 v; } fx[PWG_PF];
        #pragma unroll
        for (int pf = 0; pf < PWG_PF; ++pf) {
          fx[pf].u = *reinterpret_cast<const uint4*>(xs + (pf * 16 + l15) * xstride + cc);
          if (!cok) fx[pf].u = zero;
        }
        #pragma unroll
        for (int f = 0; f < 2; ++f)
          #pragma unroll
          for (int pf = 0; pf < PWG_PF; ++pf)
            acc[f][pf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wr[s][f].v, fx[pf].v, acc[f][pf], 0, 0, 0);
      }
    }

    // epilogue: lane (lg, l15) holds channels kb .. kb+7 of pixel pf*16 + l15
    float sc[8], bi[8];
    load8f(sb + wave * 32 + lg * 8, sc);
    load8f(sb + PWG_BK + wave * 32 + lg * 8, bi);
    #pragma unroll
    for (int pf = 0; pf < PWG_PF; ++pf) {
      float v[8];
      #pragma unroll
      for (int e = 0; e < 8; ++e)
        v[e] = acc[e >> 2][pf][e & 3] * sc[e] + bi[e];
      bf16x8 o;
      #pragma unroll
      for (int e = 0; e < 8; ++e) o.h[e] = f2b(apply_act(v[e], act));
      *reinterpret_cast<uint4*>(ys + (pf * 16 + l15) * PWG_YS + wave * 32 + lg * 8) = o.v;
    }
    __syncthreads();

    // pool: thread t adds the valid rows of channel t in row order
    if (t < PWG_BK) {
      // -ffast-math would split this chain into interleaved partial sums;
      // the contract is k_gap_fwd's one chain in row order
      #pragma clang fp reassociate(off)
      const int rv = (HW - tile0) < PWG_PT ? (HW - tile0) : PWG_PT;
      const bf16_t* col = ys + t;
      for (int r = 0; r < rv; ++r) psum += b2f(col[r * PWG_YS]);
      if (nt == 0) {                             // the image's last tile
        const int k = ktile * PWG_BK + t;
        if (k < K) p[(long)n * K + k] = f2b(psum * inv);
        psum = 0.f;
      }
    }
    n = nn;
    tile0 = nt;
  }
}

// x [N*HW][C], w [K][C], p [N][K] bf16; scale/bias fp32 [K] (both or
// neither); imgs >= 1: consecutive images per workgroup.
DDLW_EXPORT int ddlw_pw_conv_gap_fwd(const void* x, const void* w, void* p,
                                     const void* scale, const void* bias, int act,
                                     int N, int HW, int C, int K, int imgs,
                                     void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("pw_conv_gap_fwd", why); };
  if (C < 8 || C > 320 || C % 8 != 0)
    return fail("C must be a multiple of 8 in [8, 320]");
  if (K <= 0 || K % 8 != 0) return fail("K must be a positive multiple of 8");
  if (N < 0 || HW < 1) return fail("N must be >= 0 and HW >= 1");
  if ((long)N * HW >= (1l << 31)) return fail("N*HW must be below 2^31");
  if (imgs < 1) return fail("imgs must be at least 1");
  if (act < 0 || act > 2) return fail("act must be 0, 1 or 2");
  if ((scale == nullptr) != (bias == nullptr))
    return fail("scale and bias come together");
  if ((((size_t)x | (size_t)w | (size_t)scale | (size_t)bias) & 15) != 0)
    return fail("x, w, scale and bias must be 16-byte aligned");
  if (p == nullptr || ((size_t)p & 1) != 0) return fail("p must be a bf16 buffer");
  if (N == 0) return 0;
  if (imgs > N) imgs = N;
  const int ktiles = (int)cdiv(K, PWG_BK);
  const long blocks = cdiv(N, imgs) * ktiles;
  if (blocks >= (1l << 31)) return fail("grid too large");
  with_int<5, 10>(C <= 160 ? 5 : 10, [&](auto KSc) {
    hipLaunchKernelGGL((k_pw_conv_gap<decltype(KSc)::value>),
                       dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)p,
                       (const float*)scale, (const float*)bias, act, N, HW, C, K,
                       imgs, ktiles);
  });
  DDLW_CHECK_LAUNCH();
}
