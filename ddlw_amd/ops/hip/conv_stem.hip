// Dedicated stem convolution (kernel K1): 7x7 stride-2
// pad-3, C=3 -> K=64 — the one ResNet-50 conv the generic implicit-GEMM
// kernel cannot take (its K-loop needs C % 64 == 0).
//
// MI355X-native design: instead of im2col-ing a 3-channel image (6-byte
// rows; no 16-B chunks), the input is repacked ONCE per step into a
// [N][H][W + 2*HALO][4] bf16 image with a zeroed 4th channel and a zeroed
// horizontal halo, and the weights into [K][8][8][4] with zero padding.
// A 64-element K-step then factors EXACTLY as (2 r-taps) x (8 s-taps) x
// (4 channels): every staged 16-B chunk is two horizontally-adjacent
// c4 pixels, the halo removes all horizontal edge cases, and zero weight
// padding absorbs the r=7 / s=7 taps (the padded input is finite, so
// garbage*0 == 0 holds). T = 4 K-steps of BK=64 cover all 8*8*4 = 256.
//
// Tile: BM=128 x BN=64 (K=64), 4 waves (2x2), 2 LDS buffers, coalesced
// LDS-bounce epilogue (short K-loop) — the same structure as the generic
// kernel's short-K path.
#include "igemm.h"

typedef __attribute__((ext_vector_type(8))) __bf16 s_bf16x8_v;
typedef __attribute__((ext_vector_type(4))) float s_f32x4_v;

#define STEM_HALO 4

// repack: bf16 NHWC C=3 -> [N][H][W+2*HALO][4] with zero c3 + zero halo
__global__ __launch_bounds__(256) void k_stem_repack(
    const bf16_t* __restrict__ x, bf16_t* __restrict__ x4,
    long npix /* N*H*(W+2*HALO) */, int W, int Wp) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix;
       i += (long)gridDim.x * blockDim.x) {
    long row = i / Wp;          // n*H + h
    int wp = (int)(i - row * Wp);
    int w = wp - STEM_HALO;
    unsigned lo = 0, hi = 0;
    if (w >= 0 && w < W) {
      const bf16_t* src = x + (row * W + w) * 3;
      lo = (unsigned)src[0] | ((unsigned)src[1] << 16);
      hi = (unsigned)src[2];
    }
    *reinterpret_cast<uint2*>(x4 + i * 4) = make_uint2(lo, hi);
  }
}

__global__ __launch_bounds__(256) void k_conv_stem(
    const bf16_t* __restrict__ x4,   // [N][H][Wp][4]
    const bf16_t* __restrict__ w4,   // [K][256]  (8x8x4 flat)
    bf16_t* __restrict__ y,          // [M][K]
    const bf16_t* __restrict__ zpage,
    int N, int H, int Wp, int K, int Ho, int Wo, int stride, int pad,
    int nwg_swz, unsigned long long magic_wo, unsigned shift_wo,
    unsigned long long magic_ho, unsigned shift_ho,
    const float* __restrict__ ep_scale, const float* __restrict__ ep_bias,
    int ep_relu) {
  constexpr int BM = 128, BN = 64, BK = 64, T = 4;
  constexpr int WM = 64, WN = 32, MF = WM / 16, NF = WN / 16;
  constexpr int AP = BM / 32;  // 1-KiB A pieces per wave (8 rows each)
  constexpr int BP = BN / 32;
  constexpr int BUF = (BM + BN) * BK;
  constexpr int SMEM = (2 * BUF > 4 * WM * (WN + 8)) ? 2 * BUF
                                                     : 4 * WM * (WN + 8);
  __shared__ __attribute__((aligned(16))) bf16_t smem[SMEM];

  const long M = (long)N * Ho * Wo;

  int wg = blockIdx.x;
  {
    int nwg = nwg_swz;
    int q = nwg >> 3, rm = nwg & 7;
    int xcd = wg & 7, i = wg >> 3;
    wg = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + i;
  }
  const long tile_m = wg;  // tiles_n == 1 (K = 64)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  const int prow = lane >> 3;
  const int pcol8 = lane & 7;
  // swizzled chunk id + its (r_sub, s_pair) factorization (fixed per lane)
  long a_m[AP];
  int a_hb[AP];
  const bf16_t* a_base[AP];
  int a_rsub[AP], a_spair[AP];
  #pragma unroll
  for (int p = 0; p < AP; ++p) {
    int row = (wave * AP + p) * 8 + prow;
    long m = tile_m * BM + row;
    a_m[p] = m;
    int c8s = pcol8 ^ ((((wave * AP + p) & 1) << 2) | (prow >> 1));
    a_rsub[p] = c8s >> 2;    // r within the 2-tap k-step
    a_spair[p] = c8s & 3;    // pair of s taps (2 pixels = 16 B)
    if (m < M) {
      unsigned mu = (unsigned)m;
      unsigned q1 = mdiv(mu, magic_wo, shift_wo);
      int wo = (int)(mu - q1 * (unsigned)Wo);
      unsigned n_u = mdiv(q1, magic_ho, shift_ho);
      int ho = (int)(q1 - n_u * (unsigned)Ho);
      a_hb[p] = ho * stride - pad;  // input row of tap r=0
      // halo'd horizontal base: stored col = w + HALO, always >= 1
      int wb = wo * stride - pad + 2 * a_spair[p] + STEM_HALO;
      a_base[p] = x4 + (((long)(int)n_u * H + a_hb[p]) * Wp + wb) * 4;
    } else {
      a_hb[p] = -100000;
      a_base[p] = zpage;
    }
  }
  const bf16_t* b_base[BP];
  #pragma unroll
  for (int p = 0; p < BP; ++p) {
    int row = (wave * BP + p) * 8 + prow;
    int c8s = pcol8 ^ ((((wave * BP + p) & 1) << 2) | (prow >> 1));
    b_base[p] = w4 + (long)row * 256 + c8s * 8;  // row < 64 == K always
  }

  auto stage = [&](int buf, int t) {
    bf16_t* lA = smem + buf * BUF;
    bf16_t* lB = lA + BM * BK;
    #pragma unroll
    for (int p = 0; p < AP; ++p) {
      int h = a_hb[p] + 2 * t + a_rsub[p];
      bool ok = (a_m[p] < M) & (h >= 0) & (h < H);
      const bf16_t* src =
          ok ? (a_base[p] + (long)(2 * t + a_rsub[p]) * Wp * 4) : zpage;
      __builtin_amdgcn_global_load_lds(
          (const GLOBAL_AS void*)src,
          (LDS_AS void*)(lA + (wave * AP + p) * 512), 16, 0, 0);
    }
    #pragma unroll
    for (int p = 0; p < BP; ++p) {
      __builtin_amdgcn_global_load_lds(
          (const GLOBAL_AS void*)(b_base[p] + t * 64),
          (LDS_AS void*)(lB + (wave * BP + p) * 512), 16, 0, 0);
    }
  };

  s_f32x4_v acc[MF][NF];
  #pragma unroll
  for (int mi = 0; mi < MF; ++mi)
    #pragma unroll
    for (int ni = 0; ni < NF; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

  const int fr_row = lane & 15;
  const int fr_c8 = lane >> 4;

  stage(0, 0);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < T; ++t) {
    if (t + 1 < T) stage(cur ^ 1, t + 1);
    const bf16_t* lA = smem + cur * BUF;
    const bf16_t* lB = lA + BM * BK;
    #pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      s_bf16x8_v fa[MF], fb[NF];
      #pragma unroll
      for (int mi = 0; mi < MF; ++mi) {
        int row = wr * WM + mi * 16 + fr_row;
        int c8 = (kh * 4 + fr_c8) ^ ((row >> 1) & 7);
        fa[mi] = *reinterpret_cast<const s_bf16x8_v*>(lA + row * BK + c8 * 8);
      }
      #pragma unroll
      for (int ni = 0; ni < NF; ++ni) {
        int row = wc * WN + ni * 16 + fr_row;
        int c8 = (kh * 4 + fr_c8) ^ ((row >> 1) & 7);
        fb[ni] = *reinterpret_cast<const s_bf16x8_v*>(lB + row * BK + c8 * 8);
      }
      #pragma unroll
      for (int mi = 0; mi < MF; ++mi)
        #pragma unroll
        for (int ni = 0; ni < NF; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
    }
    __syncthreads();
    cur ^= 1;
  }

  // coalesced LDS-bounce epilogue (short K-loop shape)
  const int d_col = lane & 15;
  const int d_row0 = (lane >> 4) * 4;
  constexpr int WNP = WN + 8;
  bf16_t* lC = smem + wave * (WM * WNP);
  #pragma unroll
  for (int mi = 0; mi < MF; ++mi)
    #pragma unroll
    for (int ni = 0; ni < NF; ++ni)
      #pragma unroll
      for (int q = 0; q < 4; ++q)
        lC[(mi * 16 + d_row0 + q) * WNP + ni * 16 + d_col] =
            f2b(acc[mi][ni][q]);
  constexpr int CPL = WN / 8;
  constexpr int RPI = 64 / CPL;
  const int e_row = lane / CPL;
  const int e_ch = lane % CPL;
  const long m_base = tile_m * BM + wr * WM;
  const int j_base = wc * WN + e_ch * 8;
  float eps8[8], epb8[8];
  if (ep_scale) {
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      eps8[e] = ep_scale[j_base + e];
      epb8[e] = ep_bias[j_base + e];
    }
  }
  #pragma unroll
  for (int it = 0; it < WM / RPI; ++it) {
    const int row = it * RPI + e_row;
    const long m = m_base + row;
    uint4 val = *reinterpret_cast<const uint4*>(lC + row * WNP + e_ch * 8);
    if (m < M) {
      if (ep_scale) {
        // fused eval-BN apply (+relu): the stem's bn1 disappears
        unsigned* vw = &val.x;
        #pragma unroll
        for (int d = 0; d < 4; ++d) {
          float lo = b2f((bf16_t)(vw[d] & 0xffff)) * eps8[2 * d] + epb8[2 * d];
          float hi = b2f((bf16_t)(vw[d] >> 16)) * eps8[2 * d + 1] + epb8[2 * d + 1];
          if (ep_relu) { lo = fmaxf(lo, 0.f); hi = fmaxf(hi, 0.f); }
          vw[d] = (unsigned)f2b(lo) | ((unsigned)f2b(hi) << 16);
        }
      }
      *reinterpret_cast<uint4*>(y + m * K + j_base) = val;
    }
  }
}

DDLW_EXPORT int ddlw_stem_repack(const void* x, void* x4, int N, int H, int W,
                                 void* stream) {
  const int Wp = W + 2 * STEM_HALO;
  long npix = (long)N * H * Wp;
  long grid = cdiv(npix, 256);
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(k_stem_repack, dim3((int)grid), dim3(256), 0,
                     (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)x4, npix,
                     W, Wp);
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_conv_stem(const void* x4, const void* w4, void* y,
                               const void* zpage, int N, int H, int W, int K,
                               int Ho, int Wo, int stride, int pad,
                               const void* ep_scale, const void* ep_bias,
                               int ep_relu, void* stream) {
  if (K != 64 || stride != 2 || pad != 3) {
    ddlw_set_error("conv_stem: supports K=64, stride=2, pad=3 (7x7 stem)");
    return 2;
  }
  const int Wp = W + 2 * STEM_HALO;
  long M = (long)N * Ho * Wo;
  unsigned long long mg_wo, mg_ho;
  unsigned sh_wo, sh_ho;
  make_magic((unsigned)Wo, &mg_wo, &sh_wo);
  make_magic((unsigned)Ho, &mg_ho, &sh_ho);
  long grid = cdiv(M, 128);
  hipLaunchKernelGGL(k_conv_stem, dim3((int)grid), dim3(256), 0,
                     (hipStream_t)stream, (const bf16_t*)x4,
                     (const bf16_t*)w4, (bf16_t*)y, (const bf16_t*)zpage, N,
                     H, Wp, K, Ho, Wo, stride, pad, (int)grid, mg_wo, sh_wo,
                     mg_ho, sh_ho, (const float*)ep_scale,
                     (const float*)ep_bias, ep_relu);
  DDLW_CHECK_LAUNCH();
}


// ---------------------------------------------------------------------------
// Stem weight gradient: dW4[64][256] = dy^T @ im2col(x4), reduction over
// m = N*Ho*Wo split across blockIdx.z (same split-K + deterministic fp32
// slab + k_wgrad_reduce pattern as conv_wgrad.hip). The 8x8x4 zero-padded
// window is a FLAT 256-wide C dimension, so one 64x256 output tile covers
// the whole gradient and the (r, s, c) fetch reuses the fwd repack image
// (halo -> no horizontal bounds checks). Python slices the [:7][:7][:3]
// real taps out of the padded result.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) unsigned s_tr64_t;

__global__ __launch_bounds__(256) void k_stem_wgrad(
    const bf16_t* __restrict__ dy,   // [M][64]
    const bf16_t* __restrict__ x4,   // [N][H][Wp][4]
    const bf16_t* __restrict__ zpage,
    float* __restrict__ slab,        // [SPLIT][64][256]
    int N, int H, int Wp, int K, int Ho, int Wo, int stride, int pad,
    int split, long m_per_split,
    unsigned long long magic_wo, unsigned shift_wo,
    unsigned long long magic_ho, unsigned shift_ho) {
  constexpr int BK = 64, BC = 256, BM_ = 64;
  constexpr int WK = BK / 2, WC = BC / 2;
  constexpr int KF = WK / 16, CF = WC / 16;
  constexpr int PA = BK / 16 * 2;
  constexpr int PB = BC / 16 * 2;
  constexpr int TILE = BM_ * BK;
  constexpr int BUF = BM_ * (BK + BC);
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * BUF];

  const long M = (long)N * Ho * Wo;
  const int sp = blockIdx.z;
  const long m0 = (long)sp * m_per_split;
  const long m1 = (m0 + m_per_split < M) ? (m0 + m_per_split) : M;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc2 = wave & 1;

  const int s_pos = lane >> 3;
  const int s_mr = (lane >> 1) & 3;
  const int s_half = lane & 1;
  const int s_mb = (s_pos < 4) ? (2 * s_pos) : (2 * (s_pos - 4) + 1);
  const int s_mlocal = s_mb * 4 + s_mr;
  const int s_koff = s_half * 8;

  const bf16_t* dyrow[2];
  const bf16_t* xbase[2];
  int xhb[2];
  bool dv[2];

  auto decompose = [&](long mbase) {
    #pragma unroll
    for (int g = 0; g < 2; ++g) {
      long m = mbase + g * 32 + s_mlocal;
      dv[g] = m < m1;
      dyrow[g] = dv[g] ? (dy + m * K) : zpage;
      if (dv[g]) {
        unsigned mu = (unsigned)m;
        unsigned q1 = mdiv(mu, magic_wo, shift_wo);
        int wo = (int)(mu - q1 * (unsigned)Wo);
        unsigned n_u = mdiv(q1, magic_ho, shift_ho);
        int ho = (int)(q1 - n_u * (unsigned)Ho);
        xhb[g] = ho * stride - pad;
        xbase[g] = x4 + (((long)(int)n_u * H + xhb[g]) * Wp +
                         (wo * stride - pad) + STEM_HALO) * 4;
      } else {
        xhb[g] = -100000;
        xbase[g] = zpage;
      }
    }
  };

  auto stage = [&](int buf) {
    bf16_t* ldy = smem + buf * BUF;
    bf16_t* lx = ldy + TILE;
    #pragma unroll
    for (int p = wave; p < PA; p += 4) {
      const int k16 = p >> 1, g = p & 1;
      int kk = k16 * 16 + s_koff;  // K == 64, always in range
      const bf16_t* src = dv[g] ? (dyrow[g] + kk) : zpage;
      __builtin_amdgcn_global_load_lds(
          (const GLOBAL_AS void*)src, (LDS_AS void*)(ldy + p * 512), 16, 0, 0);
    }
    #pragma unroll
    for (int p = wave; p < PB; p += 4) {
      const int c16 = p >> 1, g = p & 1;
      // flat window element range [c16*16 + s_koff, +8) = 2 c4 pixels:
      // r = flat/32, s_start = ((flat%32)/4)
      const int flat = c16 * 16 + s_koff;
      const int r = flat >> 5;
      const int s_start = (flat >> 2) & 7;
      int h = xhb[g] + r;
      bool ok = dv[g] && h >= 0 && h < H;
      const bf16_t* src =
          ok ? (xbase[g] + ((long)r * Wp + s_start) * 4) : zpage;
      __builtin_amdgcn_global_load_lds(
          (const GLOBAL_AS void*)src, (LDS_AS void*)(lx + p * 512), 16, 0, 0);
    }
  };

  s_f32x4_v acc[KF][CF];
  #pragma unroll
  for (int a = 0; a < KF; ++a)
    #pragma unroll
    for (int b = 0; b < CF; ++b) acc[a][b] = {0.f, 0.f, 0.f, 0.f};

  const long nsteps = (m1 - m0 + BM_ - 1) / BM_;
  decompose(m0);
  stage(0);
  if (1 < nsteps) decompose(m0 + BM_);
  __syncthreads();

  int cur = 0;
  for (long t = 0; t < nsteps; ++t) {
    if (t + 1 < nsteps) {
      stage(cur ^ 1);
      if (t + 2 < nsteps) decompose(m0 + (t + 2) * BM_);
    }
    bf16_t* ldy = smem + cur * BUF;
    bf16_t* lx = ldy + TILE;
    #pragma unroll
    for (int mh = 0; mh < 2; ++mh) {
      s_tr64_t fk0[KF], fk1[KF], fc0[CF], fc1[CF];
      #pragma unroll
      for (int a = 0; a < KF; ++a) {
        const int k16 = (wr * WK) / 16 + a;
        unsigned addr =
            (unsigned)(unsigned long long)(const LDS_AS bf16_t*)(
                ldy + ((k16 * 2 + mh) * 8) * 64) + lane * 8;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fk0[a]) : "v"(addr));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:512"
                     : "=v"(fk1[a]) : "v"(addr));
      }
      #pragma unroll
      for (int b = 0; b < CF; ++b) {
        const int c16 = (wc2 * WC) / 16 + b;
        unsigned addr =
            (unsigned)(unsigned long long)(const LDS_AS bf16_t*)(
                lx + ((c16 * 2 + mh) * 8) * 64) + lane * 8;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fc0[b]) : "v"(addr));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:512"
                     : "=v"(fc1[b]) : "v"(addr));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      #pragma unroll
      for (int a = 0; a < KF; ++a)
        #pragma unroll
        for (int b = 0; b < CF; ++b) {
          union { struct { s_tr64_t lo, hi; } p; s_bf16x8_v v; } fa, fb;
          fa.p.lo = fk0[a]; fa.p.hi = fk1[a];
          fb.p.lo = fc0[b]; fb.p.hi = fc1[b];
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              fa.v, fb.v, acc[a][b], 0, 0, 0);
        }
    }
    __syncthreads();
    cur ^= 1;
  }

  float* out = slab + (long)sp * BK * BC;
  const int d_c = lane & 15;
  const int d_k0 = (lane >> 4) * 4;
  #pragma unroll
  for (int a = 0; a < KF; ++a)
    #pragma unroll
    for (int b = 0; b < CF; ++b) {
      int c = wc2 * WC + b * 16 + d_c;
      #pragma unroll
      for (int q = 0; q < 4; ++q) {
        int k = wr * WK + a * 16 + d_k0 + q;
        out[(long)k * BC + c] = acc[a][b][q];
      }
    }
}

DDLW_EXPORT int ddlw_stem_wgrad(const void* dy, const void* x4,
                                const void* zpage, void* slab, void* dw4,
                                int N, int H, int W, int K, int Ho, int Wo,
                                int split, void* stream) {
  if (K != 64) {
    ddlw_set_error("stem_wgrad: K must be 64");
    return 2;
  }
  const int Wp = W + 2 * STEM_HALO;
  long M = (long)N * Ho * Wo;
  unsigned long long mg_wo, mg_ho;
  unsigned sh_wo, sh_ho;
  make_magic((unsigned)Wo, &mg_wo, &sh_wo);
  make_magic((unsigned)Ho, &mg_ho, &sh_ho);
  long m_per_split = (M + split - 1) / split;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_stem_wgrad, dim3(1, 1, split), dim3(256), 0, st,
                     (const bf16_t*)dy, (const bf16_t*)x4,
                     (const bf16_t*)zpage, (float*)slab, N, H, Wp, K, Ho, Wo,
                     2, 3, split, m_per_split, mg_wo, sh_wo, mg_ho, sh_ho);
  DDLW_CHECK_LAUNCH_OR_RETURN();
  long elems = (long)K * 256;
  long g = (elems + 31) / 32;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((int)g), dim3(256), 0, st,
                     (const float*)slab, (bf16_t*)dw4, elems, split);
  DDLW_CHECK_LAUNCH();
}


// ---------------------------------------------------------------------------
// MobileNetV2 stem from uint8: preprocess_input normalize + 3x3 stride-2 pad-1
// conv (C=3 -> K=32) + folded BN + activation in one pass,
//   y[n][ho][wo][k] = act((sum_{r,s,c} xn[n][2ho-1+r][2wo-1+s][c] * w[k][r][s][c])
//                         * scale[k] + bias[k]),
//   xn = bf16(float(u8) * (1/127.5f) - 1)            (k_normalize_u8's value)
// uint8 NHWC in, bf16 NHWC out. The layer is bound by its output write
// (9.6 MB in, 51 MB out at batch 64 / 224), so nothing is staged through LDS
// and there is no barrier; the work per output vector is kept small instead.
//   - the reduction is 27 deep; zero-padded to 32 it is ONE
//     v_mfma_f32_16x16x32_bf16 step per 16 pixels x 16 channels. Operands as
//     in k_pw_conv: the weight tile is A, the pixels are B, and with its
//     weight-row order k = 8*(i>>2) + 4*f + (i&3) a lane ends up with 8
//     consecutive output channels of one pixel = one 16-byte store.
//   - reduction index kk = 9r + 3s + c: lane group lg = lane>>4 holds
//     kk = 8lg .. 8lg+7 of its pixel. Window row r is 9 contiguous input bytes
//     starting 3 bytes left of the centre column's pixel, so tap kk sits at
//     the lane-constant byte offset (r-1)*3W + (kk-9r) - 3 from the window's
//     centre pixel (2ho, 2wo), which always lies inside the image.
//   - every load is ONE BYTE (rows are 3W bytes, no alignment to assume, and
//     nothing is read past the last pixel). A tap outside the image, one of
//     the pad slots kk >= 27, or a pixel past M loads the centre byte instead
//     and is zeroed AFTER the normalize: padding is 0 in normalized space,
//     not byte 0 (= -1).
//   - the weights come repacked by the host as wp[32][32] bf16, row k holding
//     w[k][r][s][c] at 9r + 3s + c and zeros at 27..31.
// A wave owns 32 pixels x 32 channels, a block 4 waves = 128 pixels.
// ---------------------------------------------------------------------------
#define ST3_MR 2                   // 16-pixel fragments per wave
#define ST3_WAVES 4
#define ST3_BM (ST3_WAVES * ST3_MR * 16)

// what a tap needs of its pixel's window (bits of `need` / `have`)
#define ST3_TOP 1                  // row 2ho-1 inside the image
#define ST3_BOT 2                  // row 2ho+1
#define ST3_LEFT 4                 // column 2wo-1
#define ST3_RIGHT 8                // column 2wo+1
#define ST3_PIXEL 16               // the pixel itself: m < M
#define ST3_NEVER 32               // a pad slot of the reduction (kk >= 27)

// The uint8 gather, shared by every stem-u8 kernel (forward, forward with
// statistics, weight gradient) ---------------------------------------------
// The image geometry a kernel passes down, with the magic divisors of Wo, Ho.
struct St3Geom {
  int M, H, W, Ho, Wo;
  unsigned long long magic_wo, magic_ho;
  unsigned shift_wo, shift_ho;
};

// Taps kk = 8g .. 8g+7 of the reduction: byte offset from the window's centre
// pixel, and what each needs of its pixel's window.
__device__ __forceinline__ void st3_taps(int g, int W, int (&off)[8], int (&need)[8]) {
  #pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int kk = g * 8 + e;
    const int r = kk / 9, j = kk - 9 * r;  // j = 3s + c: byte in the window row
    off[e] = (r - 1) * 3 * W + j - 3;
    need[e] = ST3_PIXEL | (r == 0 ? ST3_TOP : 0) | (r == 2 ? ST3_BOT : 0) |
              (j < 3 ? ST3_LEFT : 0) | (j >= 6 ? ST3_RIGHT : 0) |
              (kk >= 27 ? ST3_NEVER : 0);
  }
}

// Output pixel m: what its window has, and its centre pixel (2ho, 2wo), which
// always lies inside the image. A pixel past M takes pixel M-1's (valid)
// address and has no ST3_PIXEL, so every tap of it is zeroed.
__device__ __forceinline__ int st3_pixel(const unsigned char* __restrict__ x,
                                         const St3Geom& g, int m,
                                         const unsigned char*& ctr) {
  const unsigned mu = (unsigned)(m < g.M ? m : g.M - 1);
  const unsigned q1 = mdiv(mu, g.magic_wo, g.shift_wo);       // n*Ho + ho
  const int wo = (int)(mu - q1 * (unsigned)g.Wo);
  const unsigned n_u = mdiv(q1, g.magic_ho, g.shift_ho);
  const int ho = (int)(q1 - n_u * (unsigned)g.Ho);
  // 2ho <= H-1 and 2wo <= W-1, and N*H*W*3 < 2^31
  ctr = x + (((int)n_u * g.H + 2 * ho) * g.W + 2 * wo) * 3;
  return (m < g.M ? ST3_PIXEL : 0) | (ho > 0 ? ST3_TOP : 0) |
         (2 * ho + 1 < g.H ? ST3_BOT : 0) | (wo > 0 ? ST3_LEFT : 0) |
         (2 * wo + 1 < g.W ? ST3_RIGHT : 0);
}

// One tap's byte: a tap the window does not have loads the centre byte.
__device__ __forceinline__ unsigned char st3_byte(const unsigned char* ctr,
                                                  int off, int need, int have) {
  return ctr[(need & ~have) == 0 ? off : 0];
}

// ... and its value: k_normalize_u8's bf16, or 0 for a tap the window lacks
// (zero padding in normalized space).
__device__ __forceinline__ bf16_t st3_value(unsigned char byte, int need, int have) {
  const float v = (float)byte * (1.f / 127.5f) - 1.f;
  return f2b((need & ~have) == 0 ? v : 0.f);
}

// Forward. STATS = false: the frozen stem with the folded-BN epilogue.
// STATS = true: the training forward — y is the raw conv output (no scale,
// bias or activation) and block b also writes the BatchNorm statistics of its
// 128 pixels, psum[b][32] = sum of y, psq[b][32] = sum of y^2 (fp32, the
// layout k_bn_finalize / k_bn_parts_fold take). As in k_pw_conv_stats the
// sums run over the bf16-ROUNDED outputs, and no sum is masked: a pixel past
// M has every tap zeroed, so its accumulators are exactly 0. No atomics: a
// lane folds its 2 pixels, a DPP row sum folds the 16 lanes, the 4 waves meet
// once in LDS and are added in wave order.
template <bool STATS>
__global__ __launch_bounds__(256) void k_stem3_u8(
    const unsigned char* __restrict__ x,   // [N][H][W][3]
    const bf16_t* __restrict__ wp,         // [32][32]
    bf16_t* __restrict__ y,                // [M][32]
    const float* __restrict__ scale, const float* __restrict__ bias, int act,
    float* __restrict__ psum, float* __restrict__ psq,   // [gridDim.x][32]
    St3Geom geo) {
  const int M = geo.M;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l15 = lane & 15;
  const int lg = lane >> 4;
  const int m0 = blockIdx.x * ST3_BM + wave * (ST3_MR * 16);

  // the lane's 8 taps: byte offset from the centre pixel, and what they need
  int off[8], need[8];
  st3_taps(lg, geo.W, off, need);

  union { uint4 u; s_bf16x8_v v; } fw[2], fx[ST3_MR];
  #pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int k = (l15 >> 2) * 8 + f * 4 + (l15 & 3);
    fw[f].u = *reinterpret_cast<const uint4*>(wp + k * 32 + lg * 8);
  }

  #pragma unroll
  for (int mi = 0; mi < ST3_MR; ++mi) {
    const unsigned char* ctr;
    const int have = st3_pixel(x, geo, m0 + mi * 16 + l15, ctr);
    bf16x8 o;
    #pragma unroll
    for (int e = 0; e < 8; ++e)
      o.h[e] = st3_value(st3_byte(ctr, off[e], need[e], have), need[e], have);
    fx[mi].u = o.v;
  }

  s_f32x4_v acc[2][ST3_MR];
  #pragma unroll
  for (int f = 0; f < 2; ++f)
    #pragma unroll
    for (int mi = 0; mi < ST3_MR; ++mi)
      acc[f][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          fw[f].v, fx[mi].v, s_f32x4_v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);

  // epilogue: lane (lg, l15) holds channels 8lg .. 8lg+7 of pixel m0 + mi*16 + l15
  if constexpr (STATS) {
    __shared__ __attribute__((aligned(16))) float red[2][ST3_WAVES][32];
    float s[8], q[8];
    #pragma unroll
    for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
    #pragma unroll
    for (int mi = 0; mi < ST3_MR; ++mi) {
      const int m = m0 + mi * 16 + l15;
      bf16x8 o;
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        o.h[e] = f2b(acc[e >> 2][mi][e & 3]);
        const float r = b2f(o.h[e]);
        s[e] += r;
        q[e] += r * r;
      }
      if (m < M) *reinterpret_cast<uint4*>(y + (long)m * 32 + lg * 8) = o.v;
    }
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      s[e] = row_sum16(s[e]);
      q[e] = row_sum16(q[e]);
    }
    if (l15 == 0) {
      float* rs = &red[0][wave][lg * 8];
      float* rq = &red[1][wave][lg * 8];
      *reinterpret_cast<float4*>(rs) = make_float4(s[0], s[1], s[2], s[3]);
      *reinterpret_cast<float4*>(rs + 4) = make_float4(s[4], s[5], s[6], s[7]);
      *reinterpret_cast<float4*>(rq) = make_float4(q[0], q[1], q[2], q[3]);
      *reinterpret_cast<float4*>(rq + 4) = make_float4(q[4], q[5], q[6], q[7]);
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 32) {
      float ts = red[0][0][t], tq = red[1][0][t];
      #pragma unroll
      for (int wv = 1; wv < ST3_WAVES; ++wv) {
        ts += red[0][wv][t];
        tq += red[1][wv][t];
      }
      psum[blockIdx.x * 32 + t] = ts;
      psq[blockIdx.x * 32 + t] = tq;
    }
    return;
  }
  float sc[8], bi[8];
  if (scale) {
    load8f(scale + lg * 8, sc);
    load8f(bias + lg * 8, bi);
  } else {
    #pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = 1.f; bi[e] = 0.f; }
  }
  #pragma unroll
  for (int mi = 0; mi < ST3_MR; ++mi) {
    const int m = m0 + mi * 16 + l15;
    if (m >= M) continue;
    bf16x8 o;
    #pragma unroll
    for (int e = 0; e < 8; ++e)
      o.h[e] = f2b(apply_act(acc[e >> 2][mi][e & 3] * sc[e] + bi[e], act));
    *reinterpret_cast<uint4*>(y + (long)m * 32 + lg * 8) = o.v;
  }
}

// output pixels of an N x H x W batch: Ho = (H-1)/2 + 1, Wo likewise
static long st3_rows(int N, int H, int W) {
  return (long)N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
}

static St3Geom st3_geom(long M, int H, int W) {
  St3Geom g;
  g.M = (int)M;
  g.H = H;
  g.W = W;
  g.Ho = (H - 1) / 2 + 1;
  g.Wo = (W - 1) / 2 + 1;
  make_magic((unsigned)g.Wo, &g.magic_wo, &g.shift_wo);
  make_magic((unsigned)g.Ho, &g.magic_ho, &g.shift_ho);
  return g;
}

// x uint8 [N][H][W][3]; wp bf16 [32][32] (w[k][r][s][c] at 9r + 3s + c, zeros
// at 27..31); y bf16 [N][Ho][Wo][32] with Ho = (H-1)/2 + 1, Wo likewise;
// scale/bias fp32 [32] (both or neither); act 0 none / 1 ReLU / 2 ReLU6.
DDLW_EXPORT int ddlw_stem3_u8_fwd_ep(const void* x, const void* wp, void* y,
                                     const void* scale, const void* bias,
                                     int act, int N, int H, int W, int C,
                                     int K, void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("stem3_u8_fwd_ep", why); };
  if (C != 3 || K != 32) return fail("takes the 3x3 stride-2 stem with C=3, K=32");
  if (N < 0 || H < 1 || W < 1) return fail("needs N >= 0 and H, W >= 1");
  if (act < 0 || act > 2) return fail("act must be 0, 1 or 2");
  if ((scale == nullptr) != (bias == nullptr))
    return fail("scale and bias come together");
  if ((((size_t)wp | (size_t)y | (size_t)scale | (size_t)bias) & 15) != 0)
    return fail("wp, y, scale and bias must be 16-byte aligned");
  const long M = st3_rows(N, H, W);
  if (M >= (1l << 31) || (long)N * H * W * 3 >= (1l << 31))
    return fail("N*Ho*Wo and N*H*W*3 must be below 2^31");
  if (M == 0) return 0;
  hipLaunchKernelGGL(k_stem3_u8<false>, dim3((unsigned)cdiv(M, ST3_BM)),
                     dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)x, (const bf16_t*)wp, (bf16_t*)y,
                     (const float*)scale, (const float*)bias, act,
                     (float*)nullptr, (float*)nullptr, st3_geom(M, H, W));
  DDLW_CHECK_LAUNCH();
}

// Partial rows ddlw_stem3_u8_fwd_stats writes per channel: one per 128-pixel
// block. Launches nothing; `stream` is there because every export outside the
// ABI test's pinned query list ends in one.
DDLW_EXPORT int ddlw_stem3_u8_nparts(long M, void* stream) {
  (void)stream;
  return (M < 0 || M >= (1l << 31)) ? -1 : (int)cdiv(M, ST3_BM);
}

// Training forward: y = conv3x3_s2_p1(normalize(x)) raw, bf16 [N][Ho][Wo][32],
// and the BN statistics partials of y, psum/psq fp32 [nparts][32] with
// nparts = ddlw_stem3_u8_nparts(N*Ho*Wo).
DDLW_EXPORT int ddlw_stem3_u8_fwd_stats(const void* x, const void* wp, void* y,
                                        void* psum, void* psq, int nparts,
                                        int N, int H, int W, int C, int K,
                                        void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("stem3_u8_fwd_stats", why); };
  if (C != 3 || K != 32) return fail("takes the 3x3 stride-2 stem with C=3, K=32");
  if (N < 0 || H < 1 || W < 1) return fail("needs N >= 0 and H, W >= 1");
  if ((((size_t)wp | (size_t)y) & 15) != 0)
    return fail("wp and y must be 16-byte aligned");
  if (psum == nullptr || psq == nullptr || (((size_t)psum | (size_t)psq) & 3) != 0)
    return fail("psum and psq must be fp32 buffers");
  const long M = st3_rows(N, H, W);
  if (M >= (1l << 31) || (long)N * H * W * 3 >= (1l << 31))
    return fail("N*Ho*Wo and N*H*W*3 must be below 2^31");
  if (nparts != ddlw_stem3_u8_nparts(M, nullptr))
    return fail("nparts must be ddlw_stem3_u8_nparts(N*Ho*Wo)");
  if (M == 0) return 0;
  hipLaunchKernelGGL(k_stem3_u8<true>, dim3((unsigned)nparts), dim3(256), 0,
                     (hipStream_t)stream, (const unsigned char*)x,
                     (const bf16_t*)wp, (bf16_t*)y, (const float*)nullptr,
                     (const float*)nullptr, 0, (float*)psum, (float*)psq,
                     st3_geom(M, H, W));
  DDLW_CHECK_LAUNCH();
}


// ---------------------------------------------------------------------------
// Stem weight gradient from the uint8 batch (no stem dgrad: it is the first
// layer):  dW[k][r][s][c] = sum_m dy[m][k] * xn[m][9r + 3s + c],  xn gathered
// by the helper above, so the normalized batch is never read or written.
// The layer is bound by reading dy (51 MB at batch 64 / 224; the byte gathers
// hit cache), and the 32 x 27 result is tiny, so this is a VALU kernel with
// the result in registers and nothing staged through LDS in its loop:
//   - a lane owns ONE pixel per step, a wave 64 consecutive pixels, and the 4
//     waves of a block take the same pixels with 8 output channels each:
//     wave w loads dy[m][8w .. 8w+7] as one 16-byte vector and the pixel's 27
//     taps as bytes, and keeps 8 x 27 fp32 accumulators. Products of two bf16
//     values are exact in fp32; only the sum rounds.
//   - block b walks the 64-pixel groups b, b + nparts, ... in that order; the
//     next group's loads are issued before the current group's 216 FMAs.
//   - a pixel past M has its dy vector zeroed and, like a tap outside the
//     image, every tap zeroed (st3_value), so it adds exactly 0; the pad
//     slots kk >= 27 are never computed.
//   - no atomics: a DPP row sum folds 16 lanes, the 4 rows of a wave meet in
//     LDS and are added in row order, and the block writes ONE partial
//     part[b][32][27]. k_stem3_u8_wgrad_sum adds the partials in a fixed
//     order and scatters kk = 9r + 3s + c into the [K][C][R][S] weight layout.
// ---------------------------------------------------------------------------
#define ST3W_PIX 64                // pixels per step: one per lane
#define ST3W_STEPS 4               // a block takes at least this many steps ...
#define ST3W_MAX_PARTS 256         // ... and there are at most this many blocks
#define ST3W_SLICES 8              // k_stem3_u8_wgrad_sum: partial slices

struct St3wLoad {
  uint4 dy;
  int have;
  unsigned char b[27];
};

__global__ __launch_bounds__(256) void k_stem3_u8_wgrad(
    const unsigned char* __restrict__ x,   // [N][H][W][3]
    const bf16_t* __restrict__ dy,         // [M][32]
    float* __restrict__ part,              // [gridDim.x][32][27]
    St3Geom geo) {
  __shared__ float red[ST3_WAVES][4][8 * 27];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int ngroups = (geo.M + ST3W_PIX - 1) / ST3W_PIX;   // M < 2^31 - 64

  int off[4][8], need[4][8];
  #pragma unroll
  for (int g = 0; g < 4; ++g) st3_taps(g, geo.W, off[g], need[g]);

  auto load = [&](int group) {
    St3wLoad l;
    const int m = group * ST3W_PIX + lane;
    const unsigned char* ctr;
    l.have = st3_pixel(x, geo, m, ctr);
    // a pixel past M reads pixel M-1's vector; compute() drops it
    l.dy = *reinterpret_cast<const uint4*>(
        dy + (long)(m < geo.M ? m : geo.M - 1) * 32 + wave * 8);
    #pragma unroll
    for (int kk = 0; kk < 27; ++kk)
      l.b[kk] = st3_byte(ctr, off[kk >> 3][kk & 7], need[kk >> 3][kk & 7], l.have);
    return l;
  };

  float acc[8][27];
  #pragma unroll
  for (int k = 0; k < 8; ++k)
    #pragma unroll
    for (int kk = 0; kk < 27; ++kk) acc[k][kk] = 0.f;

  auto compute = [&](const St3wLoad& l) {
    bf16x8 d;
    d.v = l.dy;
    if (!(l.have & ST3_PIXEL)) d.v = make_uint4(0u, 0u, 0u, 0u);
    float xn[27];
    #pragma unroll
    for (int kk = 0; kk < 27; ++kk)
      xn[kk] = b2f(st3_value(l.b[kk], need[kk >> 3][kk & 7], l.have));
    #pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float dk = b2f(d.h[k]);
      #pragma unroll
      for (int kk = 0; kk < 27; ++kk) acc[k][kk] = fmaf(dk, xn[kk], acc[k][kk]);
    }
  };

  int group = blockIdx.x;                  // gridDim.x <= ngroups
  St3wLoad cur = load(group);
  for (group += gridDim.x; group < ngroups; group += gridDim.x) {
    const St3wLoad nxt = load(group);
    compute(cur);
    cur = nxt;
  }
  compute(cur);

  const int l15 = lane & 15;
  const int lg = lane >> 4;
  #pragma unroll
  for (int k = 0; k < 8; ++k)
    #pragma unroll
    for (int kk = 0; kk < 27; ++kk) {
      const float v = row_sum16(acc[k][kk]);
      if (l15 == 0) red[wave][lg][k * 27 + kk] = v;
    }
  __syncthreads();
  // thread t: entries t, t + 256, ... of the block's [32][27]; channel k of
  // it came from wave k / 8
  for (int i = threadIdx.x; i < 32 * 27; i += 256) {
    const int wv = i / (8 * 27), j = i - wv * (8 * 27);
    float v = red[wv][0][j];
    #pragma unroll
    for (int r = 1; r < 4; ++r) v += red[wv][r][j];
    part[(long)blockIdx.x * (32 * 27) + i] = v;
  }
}

// dw[k][c][r][s] = sum_p part[p][k][9r + 3s + c]: block b takes 32 entries,
// slice j of 8 adds partials j, j + 8, ... in order, the slices meet in LDS
// and are added in slice order.
__global__ __launch_bounds__(256) void k_stem3_u8_wgrad_sum(
    const float* __restrict__ part, float* __restrict__ dw, int nparts) {
  __shared__ float red[ST3W_SLICES][32];
  const int e = threadIdx.x & 31;
  const int slice = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + e;       // k * 27 + kk; 27 blocks cover 864
  float v = 0.f;
  for (int p = slice; p < nparts; p += ST3W_SLICES) v += part[(long)p * (32 * 27) + i];
  red[slice][e] = v;
  __syncthreads();
  if (slice == 0) {
    #pragma unroll
    for (int j = 1; j < ST3W_SLICES; ++j) v += red[j][e];
    const int k = i / 27, kk = i - k * 27;
    const int r = kk / 9, s = (kk - 9 * r) / 3, c = kk - 9 * r - 3 * s;
    dw[((k * 3 + c) * 3 + r) * 3 + s] = v;
  }
}

// Partials ddlw_stem3_u8_wgrad writes: one per block, a block for every
// ST3W_STEPS groups of 64 pixels, ST3W_MAX_PARTS (one per CU) at the most.
DDLW_EXPORT int ddlw_stem3_u8_wgrad_nparts(long M, void* stream) {
  (void)stream;
  if (M < 0 || M >= (1l << 31)) return -1;
  const long n = cdiv(M, ST3W_PIX * ST3W_STEPS);
  return (int)(n < 1 ? 1 : (n > ST3W_MAX_PARTS ? ST3W_MAX_PARTS : n));
}

// x uint8 [N][H][W][3]; dy bf16 [N][Ho][Wo][32]; part fp32 scratch
// [nparts][32][27] with nparts = ddlw_stem3_u8_wgrad_nparts(N*Ho*Wo);
// dw fp32 [32][3][3][3] (K, C, R, S), every element written.
DDLW_EXPORT int ddlw_stem3_u8_wgrad(const void* x, const void* dy, void* part,
                                    void* dw, int nparts, int N, int H, int W,
                                    int C, int K, void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("stem3_u8_wgrad", why); };
  if (C != 3 || K != 32) return fail("takes the 3x3 stride-2 stem with C=3, K=32");
  if (N < 0 || H < 1 || W < 1) return fail("needs N >= 0 and H, W >= 1");
  if (((size_t)dy & 15) != 0) return fail("dy must be 16-byte aligned");
  if (part == nullptr || dw == nullptr || (((size_t)part | (size_t)dw) & 3) != 0)
    return fail("part and dw must be fp32 buffers");
  const long M = st3_rows(N, H, W);
  if (M >= (1l << 31) - ST3W_PIX || (long)N * H * W * 3 >= (1l << 31))
    return fail("N*Ho*Wo and N*H*W*3 must be below 2^31");
  if (nparts != ddlw_stem3_u8_wgrad_nparts(M, nullptr))
    return fail("nparts must be ddlw_stem3_u8_wgrad_nparts(N*Ho*Wo)");
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) {
    if (hipMemsetAsync(dw, 0, 32 * 27 * sizeof(float), st) != hipSuccess) {
      ddlw_set_error("stem3_u8_wgrad: clearing dw failed");
      return 1;
    }
    return 0;
  }
  hipLaunchKernelGGL(k_stem3_u8_wgrad, dim3((unsigned)nparts), dim3(256), 0, st,
                     (const unsigned char*)x, (const bf16_t*)dy, (float*)part,
                     st3_geom(M, H, W));
  DDLW_CHECK_LAUNCH_OR_RETURN();
  hipLaunchKernelGGL(k_stem3_u8_wgrad_sum, dim3(27), dim3(256), 0, st,
                     (const float*)part, (float*)dw, nparts);
  DDLW_CHECK_LAUNCH();
}
