// Backward of a pointwise (1x1) conv stage whose BatchNorm is FROZEN:
//   out = act(scale[k] * conv(x, W)[., k] + bias[k] (+ res)),  scale/bias the
// folded eval-mode BN, out the bf16 tensor the forward kernel wrote.
// With constant statistics the BN + activation backward is a per-element gate
// and a per-channel constant, so there is no reduction, no dz tensor and no
// mask tensor: the GEMM operand
//   g16[m][k] = gate(out[m][k]) ? bf16(fp32(dout[m][k]) * scale[k]) : 0
//   gate = 1 (act none) | 0 < out < 6 on the saved bf16 value (ReLU6)
// is formed in registers while it is loaded, one fp32 multiply and one
// round-to-nearest-even, and never written to memory. Both kernels accumulate
// in fp32 in a fixed order and use no atomics: two calls are bit-equal.
//
// k_pw_dgrad_gated — dx[m][c] = bf16(sum_k g16[m][k] * W[k][c] (+ acc[m][c])).
// k_pw_conv's GEMM (pointwise.hip) with g16 as the row operand: no LDS, no
// barrier, every fragment "8 consecutive reduction elements of one row" = one
// 16-byte global load per lane onto v_mfma_f32_16x16x32_bf16. The lane that
// loads 8 channels of dout loads the same 16 bytes of out and two float4 of
// scale. W^T [C][K] is the A operand; the host passes it transposed (the
// bf16 transpose the unfused dgrad already rebuilds per step: an A fragment
// needs 8 consecutive k of one c, which W [K][C] cannot give in one load).
// acc is the gradient that joins at the stage's input (the block's dout when
// the block has a residual), added in the epilogue before the one rounding.
// Tails as in k_pw_conv: clamped in-bounds load, zeroed register, masked
// store.
//
// k_pw_wgrad_gated — dW[k][c] = bf16(sum_m g16[m][k] * x[m][c]).
// The reduction runs over rows, the slow index of both operands, so both are
// transposed on the way into lanes: a block owns a 64 (k) x 64 (c) output
// tile and one slice of rows, and per 64-row stage its 256 threads load
// 16-byte row vectors of dout/out and of x, gate, and scatter them into LDS
// as [channel][row] (2-byte writes, the way k_head_dense_bwd transposes);
// the MFMA fragments are then 16-byte LDS reads of 8 consecutive rows of one
// channel. LDS is double-buffered: one barrier per stage. Wave w owns the 16
// k of fragment w against all 64 c (4 accumulators). x is the A operand, so
// a lane ends with 4 consecutive c of one k and a partial leaves as float4.
// Row slices write fp32 partials [nparts][K][C]; k_pw_wgrad_fold adds them
// in slice order and rounds once.
#include "pointwise.h"

// g16 of 8 channels: d = dout, o = out, sc = scale of the same 8 channels
template <int ACT>
__device__ __forceinline__ uint4 pwf_gate8(uint4 d, uint4 o, const float (&sc)[8]) {
  bf16x8 vd, vo, g;
  vd.v = d;
  vo.v = o;
  #pragma unroll
  for (int e = 0; e < 8; ++e) {
    g.h[e] = f2b(b2f(vd.h[e]) * sc[e]);
    if (ACT == 2) {
      const float ov = b2f(vo.h[e]);
      if (!(ov > 0.f && ov < 6.f)) g.h[e] = 0;
    }
  }
  return g.v;
}

template <int NP, int ACT, bool HAS_ACC>
__global__ __launch_bounds__(256) void k_pw_dgrad_gated(
    const bf16_t* __restrict__ dout, const bf16_t* __restrict__ out,
    const bf16_t* __restrict__ w_t, const float* __restrict__ scale,
    bf16_t* __restrict__ dx, const bf16_t* __restrict__ accin,
    long M, int C, int K, int ntiles) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long mtile = blockIdx.x / ntiles;
  const int ntile = blockIdx.x - (int)(mtile * ntiles);
  const int l15 = lane & 15;
  const int lg = lane >> 4;                      // 0..3: reduction group of 8
  const long m0 = mtile * PW_BM + wave * (PW_MR * 16);
  const int c0 = ntile * (NP * 32);

  long grow[PW_MR];                              // row offset into dout / out
  bool gok[PW_MR];
  #pragma unroll
  for (int mi = 0; mi < PW_MR; ++mi) {
    const long m = m0 + mi * 16 + l15;
    gok[mi] = m < M;
    grow[mi] = (gok[mi] ? m : M - 1) * K;
  }
  const bf16_t* wrow[NP][2];
  bool wok[NP][2];
  #pragma unroll
  for (int p = 0; p < NP; ++p)
    #pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int c = c0 + p * 32 + (l15 >> 2) * 8 + f * 4 + (l15 & 3);
      wok[p][f] = c < C;
      wrow[p][f] = w_t + (long)(wok[p][f] ? c : C - 1) * K;
    }

  pw_f32x4 acc[NP][2][PW_MR];
  #pragma unroll
  for (int p = 0; p < NP; ++p)
    #pragma unroll
    for (int f = 0; f < 2; ++f)
      #pragma unroll
      for (int mi = 0; mi < PW_MR; ++mi) acc[p][f][mi] = pw_f32x4{0.f, 0.f, 0.f, 0.f};

  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  for (int kb = 0; kb < K; kb += 32) {
    const int k = kb + lg * 8;
    const bool kok = k < K;
    const int kc = kok ? k : 0;
    float sc[8];
    load8f(scale + kc, sc);
    union { uint4 u; pw_bf16x8 v; } fg[PW_MR], fw[NP][2];
    #pragma unroll
    for (int mi = 0; mi < PW_MR; ++mi) {
      const uint4 d = *reinterpret_cast<const uint4*>(dout + grow[mi] + kc);
      uint4 o = zero;
      if (ACT == 2) o = *reinterpret_cast<const uint4*>(out + grow[mi] + kc);
      fg[mi].u = pwf_gate8<ACT>(d, o, sc);
      if (!(kok && gok[mi])) fg[mi].u = zero;
    }
    #pragma unroll
    for (int p = 0; p < NP; ++p)
      #pragma unroll
      for (int f = 0; f < 2; ++f) {
        fw[p][f].u = *reinterpret_cast<const uint4*>(wrow[p][f] + kc);
        if (!(kok && wok[p][f])) fw[p][f].u = zero;
      }
    #pragma unroll
    for (int p = 0; p < NP; ++p)
      #pragma unroll
      for (int f = 0; f < 2; ++f)
        #pragma unroll
        for (int mi = 0; mi < PW_MR; ++mi)
          acc[p][f][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              fw[p][f].v, fg[mi].v, acc[p][f][mi], 0, 0, 0);
  }

  // epilogue: lane (lg, l15) holds channels cb .. cb+7 of row m0 + mi*16 + l15
  #pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int cb = c0 + p * 32 + lg * 8;
    if (cb >= C) continue;
    #pragma unroll
    for (int mi = 0; mi < PW_MR; ++mi) {
      const long m = m0 + mi * 16 + l15;
      if (m >= M) continue;
      const long oi = m * C + cb;
      float v[8];
      #pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = acc[p][e >> 2][mi][e & 3];
      if constexpr (HAS_ACC) {
        bf16x8 r;
        r.v = *reinterpret_cast<const uint4*>(accin + oi);
        #pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += b2f(r.h[e]);
      }
      bf16x8 o;
      #pragma unroll
      for (int e = 0; e < 8; ++e) o.h[e] = f2b(v[e]);
      *reinterpret_cast<uint4*>(dx + oi) = o.v;
    }
  }
}

#define PWG_T 64                   // output tile: 64 k x 64 c
#define PWG_MS 64                  // rows per stage
#define PWG_LD (PWG_MS + 8)        // LDS row stride (bf16): 16-byte reads stay aligned

template <int ACT>
__global__ __launch_bounds__(256) void k_pw_wgrad_gated(
    const bf16_t* __restrict__ dout, const bf16_t* __restrict__ out,
    const bf16_t* __restrict__ x, const float* __restrict__ scale,
    float* __restrict__ part, long M, int C, int K, int ctiles, long slice) {
  __shared__ __attribute__((aligned(16))) bf16_t sg[2][PWG_T * PWG_LD];
  __shared__ __attribute__((aligned(16))) bf16_t sx[2][PWG_T * PWG_LD];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l15 = lane & 15;
  const int lg = lane >> 4;
  const int ktile = blockIdx.x / ctiles;
  const int ctile = blockIdx.x - ktile * ctiles;
  const int k0 = ktile * PWG_T, c0 = ctile * PWG_T;
  const long mbeg = (long)blockIdx.y * slice;    // < M: nparts = cdiv(M, slice)
  const long mend = mbeg + slice < M ? mbeg + slice : M;

  // staging: thread = (vector sv of 8 channels, rows sr and sr + 32)
  const int sv = tid & 7, sr = tid >> 3;
  const int kk = k0 + sv * 8, cc = c0 + sv * 8;
  const bool kok = kk < K, cok = cc < C;
  const int kc = kok ? kk : 0, ccl = cok ? cc : 0;
  float sc[8];
  load8f(scale + kc, sc);

  pw_f32x4 acc[4];
  #pragma unroll
  for (int cf = 0; cf < 4; ++cf) acc[cf] = pw_f32x4{0.f, 0.f, 0.f, 0.f};

  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  int buf = 0;
  for (long m0 = mbeg; m0 < mend; m0 += PWG_MS, buf ^= 1) {
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = sr + h * 32;
      const long m = m0 + row;
      const bool mok = m < mend;
      const long mm = mok ? m : mend - 1;
      const uint4 d = *reinterpret_cast<const uint4*>(dout + mm * K + kc);
      uint4 o = zero;
      if (ACT == 2) o = *reinterpret_cast<const uint4*>(out + mm * K + kc);
      bf16x8 g, xv;
      xv.v = *reinterpret_cast<const uint4*>(x + mm * C + ccl);
      g.v = pwf_gate8<ACT>(d, o, sc);
      if (!(mok && kok)) g.v = zero;
      if (!(mok && cok)) xv.v = zero;
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        sg[buf][(sv * 8 + e) * PWG_LD + row] = g.h[e];
        sx[buf][(sv * 8 + e) * PWG_LD + row] = xv.h[e];
      }
    }
    // one barrier per stage: a wave that passes it has finished the MFMAs of
    // the stage before, whose buffer the NEXT stage's writes reuse
    __syncthreads();
    #pragma unroll
    for (int ks = 0; ks < PWG_MS / 32; ++ks) {
      union { uint4 u; pw_bf16x8 v; } fgk, fxc;
      fgk.u = *reinterpret_cast<const uint4*>(
          &sg[buf][(wave * 16 + l15) * PWG_LD + ks * 32 + lg * 8]);
      #pragma unroll
      for (int cf = 0; cf < 4; ++cf) {
        fxc.u = *reinterpret_cast<const uint4*>(
            &sx[buf][(cf * 16 + l15) * PWG_LD + ks * 32 + lg * 8]);
        acc[cf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fxc.v, fgk.v, acc[cf], 0, 0, 0);
      }
    }
  }

  // D = x_tile^T (rows c) * g_tile (columns k): the lane holds k = l15 of
  // the wave's fragment and c = 4*lg .. 4*lg+3 of each c fragment
  const int k = k0 + wave * 16 + l15;
  if (k < K) {
    float* prow = part + ((long)blockIdx.y * K + k) * C;
    #pragma unroll
    for (int cf = 0; cf < 4; ++cf) {
      const int c = c0 + cf * 16 + lg * 4;
      if (c < C)                                 // C % 8 == 0: whole float4
        *reinterpret_cast<float4*>(prow + c) =
            make_float4(acc[cf][0], acc[cf][1], acc[cf][2], acc[cf][3]);
    }
  }
}

// dw[i] = bf16(part[0][i] + part[1][i] + ...), i over K*C. Block = 32
// elements x 8 slice groups (k_depthwise_wgrad_finalize's geometry): group pg
// adds slices pg, pg+8, ... then group 0 adds the 8 group sums in order.
__global__ __launch_bounds__(256) void k_pw_wgrad_fold(
    const float* __restrict__ part, bf16_t* __restrict__ dw, long KC, int nparts) {
  const int el = threadIdx.x & 31;
  const int pg = threadIdx.x >> 5;
  const long i = (long)blockIdx.x * 32 + el;
  float a = 0.f;
  if (i < KC)
    for (int p = pg; p < nparts; p += 8) a += part[(long)p * KC + i];
  __shared__ float la[8][32];
  la[pg][el] = a;
  __syncthreads();
  if (pg == 0 && i < KC) {
    #pragma unroll
    for (int g = 1; g < 8; ++g) a += la[g][el];
    dw[i] = f2b(a);
  }
}

// dout/out [M][K], w_t [C][K] (the transposed weight), dx/acc [M][C] bf16;
// scale fp32 [K]. act 0 none, 2 ReLU6 (out is read only then). acc may be
// null.
DDLW_EXPORT int ddlw_pw_dgrad_gated(const void* dout, const void* out,
                                    const void* w_t, const void* scale,
                                    void* dx, const void* acc, int act, long M,
                                    int C, int K, void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("pw_dgrad_gated", why); };
  if (C <= 0 || C % 8 != 0 || K <= 0 || K % 8 != 0)
    return fail("C and K must be positive multiples of 8");
  if (M < 0 || M >= (1l << 31)) return fail("M must be below 2^31");
  if (act != 0 && act != 2) return fail("act must be 0 (none) or 2 (ReLU6)");
  if (!dout || !w_t || !scale || !dx || (act == 2 && !out))
    return fail("dout, w_t, scale, dx (and out under ReLU6) are required");
  if ((((size_t)dout | (size_t)out | (size_t)w_t | (size_t)scale | (size_t)dx |
        (size_t)acc) & 15) != 0)
    return fail("pointers must be 16-byte aligned");
  if (M == 0) return 0;
  const int np = pw_pick_np(C);
  const int ntiles = (C + np * 32 - 1) / (np * 32);
  const long blocks = cdiv(M, PW_BM) * ntiles;
  if (blocks >= (1l << 31)) return fail("grid too large");
  with_int<1, 2, 3, 5, 6>(np, [&](auto NPc) {
    with_int<0, 2>(act, [&](auto ACTc) {
      with_bool(acc != nullptr, [&](auto HA) {
        hipLaunchKernelGGL(
            (k_pw_dgrad_gated<decltype(NPc)::value, decltype(ACTc)::value,
                              decltype(HA)::value>),
            dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
            (const bf16_t*)dout, (const bf16_t*)out, (const bf16_t*)w_t,
            (const float*)scale, (bf16_t*)dx, (const bf16_t*)acc, M, C, K,
            ntiles);
      });
    });
  });
  DDLW_CHECK_LAUNCH();
}

// Rows per slice of the gated wgrad, a multiple of the 64-row stage: enough
// slices for about two blocks per CU over the 64 x 64 output tiles (the 7x7
// layers, M = 3136, still fill the chip), but never so many that the fp32
// partials (nparts * K * C * 4 bytes) outweigh the bf16 operands read
// (at least M * (2K + 2C) bytes: the 112^2 layers).
static long pwg_slice(long M, int C, int K) {
  const long tiles = cdiv(K, PWG_T) * cdiv(C, PWG_T);
  const long want = cdiv(512, tiles);
  long slice = cdiv(cdiv(M, want), PWG_MS) * PWG_MS;
  const long floor_ = cdiv(cdiv(2l * K * C, (long)K + C), PWG_MS) * PWG_MS;
  if (slice < floor_) slice = floor_;
  return slice < PWG_MS ? PWG_MS : slice;
}

// number of [K][C] fp32 partials ddlw_pw_wgrad_gated writes; launches
// nothing, `stream` is unused (as in ddlw_pw_conv_nparts)
DDLW_EXPORT int ddlw_pw_wgrad_gated_nparts(long M, int C, int K, void* stream) {
  (void)stream;
  if (M <= 0 || M >= (1l << 31) || C <= 0 || K <= 0) return -1;
  return (int)cdiv(M, pwg_slice(M, C, K));
}

// dout/out [M][K], x [M][C] bf16; scale fp32 [K]; part fp32
// [ddlw_pw_wgrad_gated_nparts(M, C, K)][K][C] scratch; dw bf16 [K][C].
DDLW_EXPORT int ddlw_pw_wgrad_gated(const void* dout, const void* out,
                                    const void* x, const void* scale,
                                    void* part, void* dw, int act, long M,
                                    int C, int K, void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("pw_wgrad_gated", why); };
  if (C <= 0 || C % 8 != 0 || K <= 0 || K % 8 != 0)
    return fail("C and K must be positive multiples of 8");
  if (M <= 0 || M >= (1l << 31)) return fail("M must be positive and below 2^31");
  if (act != 0 && act != 2) return fail("act must be 0 (none) or 2 (ReLU6)");
  if (!dout || !x || !scale || !part || !dw || (act == 2 && !out))
    return fail("dout, x, scale, part, dw (and out under ReLU6) are required");
  if ((((size_t)dout | (size_t)out | (size_t)x | (size_t)scale |
        (size_t)part) & 15) != 0)
    return fail("pointers must be 16-byte aligned");
  const long slice = pwg_slice(M, C, K);
  const int nparts = (int)cdiv(M, slice);
  const int ctiles = (int)cdiv(C, PWG_T);
  const long tiles = cdiv(K, PWG_T) * ctiles;
  if (tiles >= (1l << 31) || nparts > 65535) return fail("grid too large");
  with_int<0, 2>(act, [&](auto ACTc) {
    hipLaunchKernelGGL((k_pw_wgrad_gated<decltype(ACTc)::value>),
                       dim3((unsigned)tiles, (unsigned)nparts), dim3(256), 0,
                       (hipStream_t)stream, (const bf16_t*)dout,
                       (const bf16_t*)out, (const bf16_t*)x,
                       (const float*)scale, (float*)part, M, C, K, ctiles,
                       slice);
  });
  DDLW_CHECK_LAUNCH_OR_RETURN();
  const long KC = (long)K * C;
  hipLaunchKernelGGL(k_pw_wgrad_fold, dim3((unsigned)cdiv(KC, 32)), dim3(256), 0,
                     (hipStream_t)stream, (const float*)part, (bf16_t*)dw, KC,
                     nparts);
  DDLW_CHECK_LAUNCH();
}
