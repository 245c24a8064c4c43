// MFMA implicit-GEMM convolution for CDNA4 (gfx950), NHWC bf16, fp32 accum.
//
// GEMM view (kernels K1-K3 of SURVEY.md §2.4; the north star's "conv2d
// fwd/bwd ... MFMA implicit-GEMM with LDS im2col tiles"):
//   O[M=N*Ho*Wo][Cout] = im2col(x)[M][R*S*C] @ W[Cout][R*S*C]^T
// Weight layout = channels_last flat [Cout][R][S][C] (B^T GEMM input).
// Loop order r,s outer / C-chunks inner, so every staged 16-B chunk is 8
// consecutive channels of one pixel (no divisions in the hot loop).
//
// dgrad(stride=1) reuses THIS kernel with flipped/transposed weights
// (dx = conv_s1(dy, W'); W'[c][r'][s'][k] = W[k][R-1-r'][S-1-s'][c],
// pad' = R-1-pad), so fwd and dgrad share one MFMA path.
//
// Structure = the cdna_hip_programming.md §5 "step-3" ladder shape:
//   - BK=64 K-steps, TWO LDS buffers, async global->LDS via
//     global_load_lds_dwordx4 (1 KiB per wave-instruction), plain
//     __syncthreads() per step (hipcc adds the vmcnt drain);
//   - LDS image is lane-linear [rows][64] bf16 (glds writes base+lane*16),
//     so the bank swizzle lives on the SOURCE address and the fragment
//     read: chunk col8 ^= (row>>1)&7  (rule 21: same involution both sides);
//   - im2col padding/tile edges are handled by redirecting the per-lane
//     glds source to a zero page (glds has no predication);
//   - 2x2 wave grid, each wave (BM/2 x BN/2) of 16x16 fragments,
//     v_mfma_f32_16x16x32_bf16, two K-halves per BK=64 step;
//   - XCD-aware bijective workgroup swizzle (L2 tile locality).
#include "igemm.h"
#include <cstdlib>
#include <type_traits>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_v;
typedef __attribute__((ext_vector_type(4))) float f32x4_v;
typedef __attribute__((ext_vector_type(16))) float f32x16_v;

// BN-stats fusion: the conv epilogue already holds every output value in
// registers — accumulating per-channel sum/sumsq here saves the separate
// k_bn_stats full read of the conv output (~1.2 ms/step on ResNet-50 b256).
// Each (tile_m, wr) wave-row writes ONE deterministic partial row
// [nparts][K]; nparts = grid_m * (BM/WM); k_bn_finalize reduces them.
// Values are accumulated bf16-rounded so the stats match the unfused
// k_bn_stats(y) numerics exactly.
template <int MF, int NF, int BM, int BN, int WM, int WN, typename ACC>
__device__ __forceinline__ void bn_partials_16(
    const ACC& acc, float* __restrict__ bn_ps, float* __restrict__ bn_pq,
    long tile_m, int tile_n, int wr, int wc, long M, int K) {
  const int lane = threadIdx.x & 63;
  const int d_col = lane & 15;
  const int d_row0 = (lane >> 4) * 4;
  float s[NF], q[NF];
  #pragma unroll
  for (int ni = 0; ni < NF; ++ni) { s[ni] = 0.f; q[ni] = 0.f; }
  #pragma unroll
  for (int mi = 0; mi < MF; ++mi)
    #pragma unroll
    for (int ni = 0; ni < NF; ++ni)
      #pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        long m = tile_m * BM + (long)wr * WM + mi * 16 + d_row0 + qq;
        if (m < M) {
          union { unsigned i; float f; } cv;
          cv.i = (unsigned)f2b(acc[mi][ni][qq]) << 16;
          s[ni] += cv.f;
          q[ni] += cv.f * cv.f;
        }
      }
  #pragma unroll
  for (int ni = 0; ni < NF; ++ni) {
    s[ni] += __shfl_xor(s[ni], 16, 64);
    s[ni] += __shfl_xor(s[ni], 32, 64);
    q[ni] += __shfl_xor(q[ni], 16, 64);
    q[ni] += __shfl_xor(q[ni], 32, 64);
  }
  if (lane < 16) {
    const long prow_ = tile_m * (BM / WM) + wr;
    #pragma unroll
    for (int ni = 0; ni < NF; ++ni) {
      int j = tile_n * BN + wc * WN + ni * 16 + d_col;
      if (j < K) {
        bn_ps[prow_ * K + j] = s[ni];
        bn_pq[prow_ * K + j] = q[ni];
      }
    }
  }
}

// BN-BACKWARD reduce fusion: a conv dgrad's epilogue already holds the dy
// of the NEXT BatchNorm backward in registers — accumulating the masked
// (dbeta, dgamma) partials here removes k_bn_bwd_reduce's re-read of dy
// (SURVEY.md §2.4 fused-op mandate; reduce was ~9% of the train step).
//   part_db = sum(mask * v),  part_dg = sum(mask * v * (x - mean) * rstd)
template <int MF, int NF, int BM, int BN, int WM, int WN, typename ACC,
          typename OutRow>
__device__ __forceinline__ void bnb_partials_16(
    const ACC& acc, const bf16_t* __restrict__ accp,
    const unsigned char* __restrict__ accmask,
    const bf16_t* __restrict__ bx, const unsigned char* __restrict__ bmask,
    const float* __restrict__ bmean, const float* __restrict__ brstd,
    float* __restrict__ p_db, float* __restrict__ p_dg,
    long tile_m, int tile_n, int wr, int wc, long M, int K, OutRow out_row) {
  const int lane = threadIdx.x & 63;
  const int d_col = lane & 15;
  const int d_row0 = (lane >> 4) * 4;
  float s[NF], q[NF], mn[NF], rs[NF];
  #pragma unroll
  for (int ni = 0; ni < NF; ++ni) {
    int j = tile_n * BN + wc * WN + ni * 16 + d_col;
    s[ni] = 0.f;
    q[ni] = 0.f;
    mn[ni] = (j < K) ? bmean[j] : 0.f;
    rs[ni] = (j < K) ? brstd[j] : 0.f;
  }
  #pragma unroll
  for (int mi = 0; mi < MF; ++mi)
    #pragma unroll
    for (int ni = 0; ni < NF; ++ni) {
      int j = tile_n * BN + wc * WN + ni * 16 + d_col;
      if (j >= K) continue;
      #pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        long m = tile_m * BM + (long)wr * WM + mi * 16 + d_row0 + qq;
        if (m < M) {
          long oi = out_row(m) * K + j;
          float v = acc[mi][ni][qq];
          if (accp) {
            union { unsigned i; float f; } ca;
            ca.i = (unsigned)accp[oi] << 16;
            if (accmask && !((accmask[oi >> 3] >> (j & 7)) & 1)) ca.f = 0.f;
            v += ca.f;
          }
          union { unsigned i; float f; } cv;
          cv.i = (unsigned)f2b(v) << 16;  // the stored bf16 value
          bool on = true;
          if (bmask)
            on = (bmask[oi >> 3] >> (j & 7)) & 1;
          if (on) {
            union { unsigned i; float f; } cx;
            cx.i = (unsigned)bx[oi] << 16;
            s[ni] += cv.f;
            q[ni] += cv.f * (cx.f - mn[ni]) * rs[ni];
          }
        }
      }
    }
  #pragma unroll
  for (int ni = 0; ni < NF; ++ni) {
    s[ni] += __shfl_xor(s[ni], 16, 64);
    s[ni] += __shfl_xor(s[ni], 32, 64);
    q[ni] += __shfl_xor(q[ni], 16, 64);
    q[ni] += __shfl_xor(q[ni], 32, 64);
  }
  if (lane < 16) {
    const long prow_ = tile_m * (BM / WM) + wr;
    #pragma unroll
    for (int ni = 0; ni < NF; ++ni) {
      int j = tile_n * BN + wc * WN + ni * 16 + d_col;
      if (j < K) {
        p_db[prow_ * K + j] = s[ni];
        p_dg[prow_ * K + j] = q[ni];
      }
    }
  }
}

// stride-2 dgrad, merged parity classes: blockIdx.y picks one of four
// (h%2, w%2) output-parity classes, each a small stride-1 conv of dy with
// its own gathered taps and scattered output offset. One launch keeps the
// short-K classes (1 tap) resident WITH the 4-tap class instead of four
// serialized latency-bound launches.
struct S2Class {
  long woff;   // offset into the concatenated per-class weights
  long yoff;   // output element offset ((dh*iw + dw) * C)
  int R, S;    // taps of this class
};
struct S2Quad {
  S2Class c[4];
};

// ACC_EARLY (bounce epilogue only): add acc to the fp32 accumulators before
// the bounce instead of to the bf16 values after it — see the epilogue.
// MASKED: acc_mask is honoured. A template flag so that the unmasked
// instantiations keep exactly the code (and the fp32 summation order of the
// BN partials) they had.
// PF > 0 (bounce epilogue only): the epilogue's side reads — acc, acc_mask,
// bnb_x, bnb_mask — are issued PF store-loop iterations ahead of their use,
// and with ACC_EARLY the add is taken from a coalesced fp32 bounce instead
// of the per-element gather. Lane -> (row, chunk) mapping, the ascending-row
// order of each lane's partial sums and the shuffle tree are those of PF = 0,
// so both give the same bits. A template flag for the same reason as MASKED.
template <int BM, int BN, bool EPI_LDS, int BUFS, bool M32EN = true,
          bool ACC_EARLY = false, bool MASKED = false, int PF = 0>
__global__ __launch_bounds__(256) void k_conv_fwd_igemm(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ y, const bf16_t* __restrict__ zpage,
    int N, int H, int W_, int C, int K, int Ho, int Wo,
    int R, int S, int stride, int pad, int nwg_swz,
    int oH, int oW, int oS,  // output scatter: flat out row = (n*oH + ho*oS)*oW + wo*oS
    unsigned long long magic_wo, unsigned shift_wo,
    unsigned long long magic_ho, unsigned shift_ho,
    const bf16_t* __restrict__ accp,   // optional epilogue accumulate input
    const unsigned char* __restrict__ acc_mask,  // optional: accp counts only
                                       // where its bit is set (1 B / 8 ch)
    float* __restrict__ bn_ps,         // optional BN partial sums [nparts][K]
    float* __restrict__ bn_pq,         // optional BN partial sumsq
    const bf16_t* __restrict__ bnb_x,  // != null: BN-BWD mode — partials
    const unsigned char* __restrict__ bnb_mask,  // become (dbeta, dgamma)
    const float* __restrict__ bnb_mean,
    const float* __restrict__ bnb_rstd,
    const float* __restrict__ ep_scale = nullptr,  // eval-BN fold:
    const float* __restrict__ ep_bias = nullptr,   //  y = relu?(v*s+b [+acc])
    int ep_relu = 0,
    int s2_merged = 0, S2Quad quad = {}) {
  if (s2_merged) {
    const S2Class& cc = quad.c[blockIdx.y];
    w += cc.woff;
    y += cc.yoff;
    R = cc.R;
    S = cc.S;
  }
  // accp != nullptr: y = conv + accp (read at the output index). Used to
  // fuse the residual-join gradient add (d_block_input = conv1_dgrad +
  // d_identity) into the dgrad epilogue — saves the engine's separate
  // 3-pass elementwise add (read A, read B, write C) per ResNet join.
  // acc_mask != nullptr: the add-input is taken as (bit ? accp : +0) with the
  // bn_apply relu-mask layout (byte oi>>3, bit j&7) — the join reads dy and
  // bn3's mask instead of a materialised masked copy of dy.
  constexpr int BK = 64;
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int MF = WM / 16, NF = WN / 16;
  constexpr int AP = BM / 32;  // 1-KiB A pieces per wave (8 rows each)
  constexpr int BP = BN / 32;  // 1-KiB B pieces per wave
  constexpr int BUF = (BM + BN) * BK;  // bf16 elements per buffer
  // BUFS=1 for single-K-step shapes (no pipeline to double-buffer; half the
  // LDS -> twice the resident blocks on these latency-bound 1x1 layers);
  // the epilogue LDS bounce needs up to 4*WM*(WN+8) elements.
  constexpr int SMEM = (BUFS * BUF > 4 * (BM / 2) * (BN / 2 + 8))
                           ? BUFS * BUF
                           : 4 * (BM / 2) * (BN / 2 + 8);

  __shared__ __attribute__((aligned(16))) bf16_t smem[SMEM];

  const long M = (long)N * Ho * Wo;
  const int tiles_n = (K + BN - 1) / BN;

  // bijective XCD swizzle: consecutive swizzled ids land on one XCD
  int wg = blockIdx.x;
  {
    int nwg = nwg_swz;
    int q = nwg >> 3, rm = nwg & 7;
    int xcd = wg & 7, i = wg >> 3;
    wg = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + i;
  }
  const int tile_n = wg % tiles_n;
  const long tile_m = wg / tiles_n;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  // ---- per-thread staging geometry (fixed across k-steps) -----------------
  // piece pa = wave*AP + p covers LDS rows pa*8..pa*8+7; this lane's row/col:
  const int prow = lane >> 3;          // row within piece
  const int pcol8 = lane & 7;          // dest col8 within row
  long a_m[AP];
  int a_hb[AP], a_wb[AP];
  const bf16_t* a_base[AP];
  #pragma unroll
  for (int p = 0; p < AP; ++p) {
    int row = (wave * AP + p) * 8 + prow;
    long m = tile_m * BM + row;
    a_m[p] = m;
    if (m < M) {
      unsigned mu = (unsigned)m;
      unsigned q1 = mdiv(mu, magic_wo, shift_wo);     // m / Wo
      int wo = (int)(mu - q1 * (unsigned)Wo);
      unsigned n_u = mdiv(q1, magic_ho, shift_ho);    // (m/Wo) / Ho
      int ho = (int)(q1 - n_u * (unsigned)Ho);
      int n = (int)n_u;
      a_hb[p] = ho * stride - pad;
      a_wb[p] = wo * stride - pad;
      // source chunk col8' = dest col8 ^ ((row>>1)&7): the b128 bank row
      // is 256 B = TWO 128-B LDS rows, so an XOR keyed on row&7 leaves a
      // 2-way conflict between rows r and r+8 of a 16-row fragment group;
      // keying on (row>>1)&7 is conflict-free for 16- and 32-row groups
      a_base[p] = x + (((long)n * H + a_hb[p]) * W_ + a_wb[p]) * C +
                  (pcol8 ^ ((((wave * AP + p) & 1) << 2) | (prow >> 1))) * 8;
    } else {
      a_hb[p] = -100000;
      a_wb[p] = -100000;
      a_base[p] = zpage;
    }
  }
  const long KRS = (long)R * S * C;
  const bf16_t* b_base[BP];
  bool b_ok[BP];
  #pragma unroll
  for (int p = 0; p < BP; ++p) {
    int row = (wave * BP + p) * 8 + prow;
    int j = tile_n * BN + row;
    b_ok[p] = j < K;
    b_base[p] = b_ok[p]
        ? (w + (long)j * KRS +
           (pcol8 ^ ((((wave * BP + p) & 1) << 2) | (prow >> 1))) * 8)
        : zpage;
  }

  // ---- staging: one glds per piece into buffer `b` for k-step (r,s,ck)
  auto stage = [&](int buf, int r, int s, int ck) {
    bf16_t* lA = smem + buf * BUF;
    bf16_t* lB = lA + BM * BK;
    const long aoff = ((long)r * W_ + s) * C + ck;
    #pragma unroll
    for (int p = 0; p < AP; ++p) {
      int h = a_hb[p] + r, ww = a_wb[p] + s;
      bool ok = (a_m[p] < M) & (h >= 0) & (h < H) & (ww >= 0) & (ww < W_);
      const bf16_t* src = ok ? (a_base[p] + aoff) : zpage;
      __builtin_amdgcn_global_load_lds(
          (const GLOBAL_AS void*)src,
          (LDS_AS void*)(lA + (wave * AP + p) * 512), 16, 0, 0);
    }
    const long boff = ((long)r * S + s) * C + ck;
    #pragma unroll
    for (int p = 0; p < BP; ++p) {
      const bf16_t* src = b_ok[p] ? (b_base[p] + boff) : zpage;
      __builtin_amdgcn_global_load_lds(
          (const GLOBAL_AS void*)src,
          (LDS_AS void*)(lB + (wave * BP + p) * 512), 16, 0, 0);
    }
  };

  // MFMA shape: 32x32x16 when the per-wave tile is >=32 in both dims
  // (2382 vs 2075 TF/s ubench ceiling over 16x16x32); 16x16x32 otherwise.
  constexpr bool M32 = M32EN && (WM >= 32) && (WN >= 32);
  constexpr int MF2 = M32 ? WM / 32 : 1, NF2 = M32 ? WN / 32 : 1;
  f32x4_v acc[M32 ? 1 : MF][M32 ? 1 : NF];
  f32x16_v acc2[MF2][NF2];
  if constexpr (M32) {
    #pragma unroll
    for (int mi = 0; mi < MF2; ++mi)
      #pragma unroll
      for (int ni = 0; ni < NF2; ++ni)
        #pragma unroll
        for (int e = 0; e < 16; ++e) acc2[mi][ni][e] = 0.f;
  } else {
    #pragma unroll
    for (int mi = 0; mi < MF; ++mi)
      #pragma unroll
      for (int ni = 0; ni < NF; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};
  }

  const int fr_row = lane & 15;
  const int fr_c8 = lane >> 4;  // col8 base per k-half: kh*4 + (lane>>4)
  const int fr_row32 = lane & 31;
  const int fr_q8 = lane >> 5;  // k-eighth within a 16-K quarter

  const int csteps = C / BK;
  const int T = R * S * csteps;
  int r2 = 0, s2 = 0, ck2 = 0;
  auto advance = [&]() {
    ck2 += BK;
    if (ck2 >= C) {
      ck2 = 0;
      if (++s2 >= S) { s2 = 0; ++r2; }
    }
  };

  stage(0, r2, s2, ck2);
  advance();
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < T; ++t) {
    if (BUFS > 1 && t + 1 < T) {
      stage(cur ^ 1, r2, s2, ck2);
      advance();
    }
    bf16_t* lA = smem + cur * BUF;
    bf16_t* lB = lA + BM * BK;
    if constexpr (M32) {
      // four 16-K quarters per BK=64; A/B fragment per lane: 8 bf16 at
      // [row = lane&31][k = kq*16 + (lane>>5)*8]
      #pragma unroll
      for (int kq = 0; kq < 4; ++kq) {
        bf16x8_v fa[MF2], fb[NF2];
        #pragma unroll
        for (int mi = 0; mi < MF2; ++mi) {
          int row = wr * WM + mi * 32 + fr_row32;
          int c8 = (kq * 2 + fr_q8) ^ ((row >> 1) & 7);
          fa[mi] = *reinterpret_cast<const bf16x8_v*>(lA + row * BK + c8 * 8);
        }
        #pragma unroll
        for (int ni = 0; ni < NF2; ++ni) {
          int row = wc * WN + ni * 32 + fr_row32;
          int c8 = (kq * 2 + fr_q8) ^ ((row >> 1) & 7);
          fb[ni] = *reinterpret_cast<const bf16x8_v*>(lB + row * BK + c8 * 8);
        }
        #pragma unroll
        for (int mi = 0; mi < MF2; ++mi)
          #pragma unroll
          for (int ni = 0; ni < NF2; ++ni)
            acc2[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                fa[mi], fb[ni], acc2[mi][ni], 0, 0, 0);
      }
    } else {
      #pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        bf16x8_v fa[MF], fb[NF];
        #pragma unroll
        for (int mi = 0; mi < MF; ++mi) {
          int row = wr * WM + mi * 16 + fr_row;
          int c8 = (kh * 4 + fr_c8) ^ ((row >> 1) & 7);
          fa[mi] = *reinterpret_cast<const bf16x8_v*>(lA + row * BK + c8 * 8);
        }
        #pragma unroll
        for (int ni = 0; ni < NF; ++ni) {
          int row = wc * WN + ni * 16 + fr_row;
          int c8 = (kh * 4 + fr_c8) ^ ((row >> 1) & 7);
          fb[ni] = *reinterpret_cast<const bf16x8_v*>(lB + row * BK + c8 * 8);
        }
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int mi = 0; mi < MF; ++mi)
          #pragma unroll
          for (int ni = 0; ni < NF; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    __syncthreads();
    if (BUFS > 1) cur ^= 1;
  }

  // ---- epilogue. Two variants:
  // EPI_LDS=false: direct scalar stores from the D lane map (col = lane&15,
  //   row = (lane>>4)*4 + q) — measured fastest when the K-loop is long
  //   (store tail amortized/hidden across resident blocks);
  // EPI_LDS=true (short K-loop shapes): LDS bounce -> line-coalesced
  //   dwordx4 stores with lane -> (row = lane/CPL, chunk = lane%CPL): every
  //   wave-instruction covers whole consecutive 128-B rows.
  const int d_col = lane & 15;
  const int d_row0 = (lane >> 4) * 4;
  auto out_row = [&](long m) -> long {
    if (oS == 1) return m;  // identity scatter (normal fwd)
    unsigned mu = (unsigned)m;
    unsigned q1 = mdiv(mu, magic_wo, shift_wo);
    int wo = (int)(mu - q1 * (unsigned)Wo);
    unsigned n_u = mdiv(q1, magic_ho, shift_ho);
    int ho = (int)(q1 - n_u * (unsigned)Ho);
    return ((long)(int)n_u * oH + (long)ho * oS) * oW + (long)wo * oS;
  };
  // 32x32 D map: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
  const int d_col32 = lane & 31;
  const int d_rbase32 = 4 * (lane >> 5);
  auto b2f = [](bf16_t u) -> float {
    union { unsigned i; float f; } cvt;
    cvt.i = (unsigned)u << 16;
    return cvt.f;
  };
  if (!EPI_LDS) {
    if constexpr (M32) {
      #pragma unroll
      for (int mi = 0; mi < MF2; ++mi) {
        #pragma unroll
        for (int ni = 0; ni < NF2; ++ni) {
          int j = tile_n * BN + wc * WN + ni * 32 + d_col32;
          if (j >= K) continue;
          #pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            int row = (reg & 3) + 8 * (reg >> 2) + d_rbase32;
            long m = tile_m * BM + wr * WM + mi * 32 + row;
            if (m < M) {
              long oi = out_row(m) * K + j;
              float v = acc2[mi][ni][reg];
              if (accp) v += b2f(accp[oi]);
              y[oi] = f2b(v);
            }
          }
        }
      }
    } else {
      float eps_[NF], epb_[NF];
      if (ep_scale) {
        #pragma unroll
        for (int ni = 0; ni < NF; ++ni) {
          int j = tile_n * BN + wc * WN + ni * 16 + d_col;
          eps_[ni] = (j < K) ? ep_scale[j] : 0.f;
          epb_[ni] = (j < K) ? ep_bias[j] : 0.f;
        }
      }
      #pragma unroll
      for (int mi = 0; mi < MF; ++mi) {
        #pragma unroll
        for (int ni = 0; ni < NF; ++ni) {
          int j = tile_n * BN + wc * WN + ni * 16 + d_col;
          if (j >= K) continue;
          #pragma unroll
          for (int q = 0; q < 4; ++q) {
            long m = tile_m * BM + wr * WM + mi * 16 + d_row0 + q;
            if (m < M) {
              long oi = out_row(m) * K + j;
              float v = acc[mi][ni][q];
              if constexpr (MASKED) {
                float a = b2f(accp[oi]);
                if (!((acc_mask[oi >> 3] >> (j & 7)) & 1)) a = 0.f;
                v += a;
              } else {
                if (ep_scale) v = v * eps_[ni] + epb_[ni];
                if (accp) v += b2f(accp[oi]);
                if (ep_relu) v = fmaxf(v, 0.f);
              }
              y[oi] = f2b(v);
            }
          }
        }
      }
      if (bn_ps) {
        if (bnb_x)
          bnb_partials_16<MF, NF, BM, BN, WM, WN>(
              acc, accp, MASKED ? acc_mask : nullptr, bnb_x, bnb_mask, bnb_mean, bnb_rstd, bn_ps,
              bn_pq, tile_m, tile_n, wr, wc, M, K, out_row);
        else
          bn_partials_16<MF, NF, BM, BN, WM, WN>(acc, bn_ps, bn_pq, tile_m,
                                                 tile_n, wr, wc, M, K);
      }
    }
    return;
  }
  constexpr int WNP = WN + 8;  // pad off the bank power-of-two
  bf16_t* lC = smem + wave * (WM * WNP);
  // A long-K shape (T > 4) bounces only because bnb forces it; on its own
  // it takes the direct epilogue, which adds acc in fp32 BEFORE the one bf16
  // rounding. Keep that order here, so dx does not depend on whether the
  // reduce partials ride along: add acc to the accumulators now (the same
  // per-element reads the direct epilogue does) and skip the add below. Its
  // own instantiation (the launcher picks it for acc + bnb at T > 4): as a
  // runtime branch it cost the single-K-step tiles a wave of occupancy.
  constexpr bool acc_early = ACC_EARLY && !M32;
  // PF > 0: the side reads of iteration `it` of the store loop below are
  // issued PF iterations ahead (the first PF groups right here, before the
  // accumulators go to LDS: the addresses depend on the tile indices only).
  // Each load keeps the predicate of the load it replaces. F32B: the early
  // add is taken from an fp32 bounce of the accumulators (two halves of
  // WM/2 rows, the wave's own LDS region) with the same coalesced mapping,
  // not from the per-element gather.
  constexpr bool F32B = acc_early && PF > 0;
  constexpr int NIT = WM / (64 / (WN / 8));  // store-loop iterations
  constexpr int PFD = PF < NIT ? PF : NIT;
  constexpr int PFN = PF > 0 ? NIT : 1;
  uint4 pf_a[PFN], pf_x[PFN];
  unsigned pf_am[PFN], pf_xm[PFN];
  auto pf_issue = [&](int it) {
    const int row = it * (64 / (WN / 8)) + lane / (WN / 8);
    const long m = tile_m * BM + wr * WM + row;
    const int jb = tile_n * BN + wc * WN + (lane % (WN / 8)) * 8;
    if (m < M && jb + 8 <= K) {
      const long o = out_row(m) * K + jb;
      if (accp && (!acc_early || F32B)) {
        pf_a[it] = *reinterpret_cast<const uint4*>(accp + o);
        if constexpr (MASKED) pf_am[it] = acc_mask[o >> 3];
      }
      if (bn_ps && bnb_x) {
        pf_x[it] = *reinterpret_cast<const uint4*>(bnb_x + o);
        pf_xm[it] = bnb_mask ? bnb_mask[o >> 3] : 0xffu;
      }
    }
  };
  // the per-channel bnb constants go first: loads return in order, and the
  // first store-loop iteration needs them
  float pf_bnm[PF > 0 ? 8 : 1], pf_bnr[PF > 0 ? 8 : 1];
  if constexpr (PF > 0) {
    if (bn_ps && bnb_x) {
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        int j = tile_n * BN + wc * WN + (lane % (WN / 8)) * 8 + e;
        pf_bnm[e] = (j < K) ? bnb_mean[j] : 0.f;
        pf_bnr[e] = (j < K) ? bnb_rstd[j] : 0.f;
      }
    }
    #pragma unroll
    for (int it = 0; it < PFD; ++it) pf_issue(it);
  }
  if constexpr (F32B) {
    // written half by half inside the store loop
  } else if constexpr (M32) {
    #pragma unroll
    for (int mi = 0; mi < MF2; ++mi)
      #pragma unroll
      for (int ni = 0; ni < NF2; ++ni)
        #pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          int row = (reg & 3) + 8 * (reg >> 2) + d_rbase32;
          lC[(mi * 32 + row) * WNP + ni * 32 + d_col32] =
              f2b(acc2[mi][ni][reg]);
        }
  } else {
    if constexpr (acc_early) {
        #pragma unroll
        for (int mi = 0; mi < MF; ++mi) {
          #pragma unroll
          for (int ni = 0; ni < NF; ++ni) {
            int j = tile_n * BN + wc * WN + ni * 16 + d_col;
            if (j >= K) continue;
            #pragma unroll
            for (int q = 0; q < 4; ++q) {
              long m = tile_m * BM + wr * WM + mi * 16 + d_row0 + q;
              if (m < M) {
                long oi = out_row(m) * K + j;
                float a = b2f(accp[oi]);
                if constexpr (MASKED) {
                  if (!((acc_mask[oi >> 3] >> (j & 7)) & 1)) a = 0.f;
                }
                acc[mi][ni][q] += a;
              }
            }
          }
        }
    }
    #pragma unroll
    for (int mi = 0; mi < MF; ++mi)
      #pragma unroll
      for (int ni = 0; ni < NF; ++ni)
        #pragma unroll
        for (int q = 0; q < 4; ++q)
          lC[(mi * 16 + d_row0 + q) * WNP + ni * 16 + d_col] =
              f2b(acc[mi][ni][q]);
  }
  // wave-private region: lgkmcnt ordering suffices, no barrier needed
  constexpr int CPL = WN / 8;        // 16-B chunks per output row
  constexpr int RPI = 64 / CPL;      // rows covered per store instruction
  const int e_row = lane / CPL;      // row within the iteration group
  const int e_ch = lane % CPL;       // chunk within the row
  const long m_base = tile_m * BM + wr * WM;
  const int j_base = tile_n * BN + wc * WN + e_ch * 8;
  float eps8[8], epb8[8];
  if (ep_scale) {
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      int j = j_base + e;
      eps8[e] = (j < K) ? ep_scale[j] : 0.f;
      epb8[e] = (j < K) ? ep_bias[j] : 0.f;
    }
  }
  // apply the eval-BN fold (+acc +relu) to one bf16 element
  auto ep_apply = [&](bf16_t v, int e, float accv) -> bf16_t {
    float f = b2f(v) * eps8[e] + epb8[e] + accv;
    if (ep_relu) f = fmaxf(f, 0.f);
    return f2b(f);
  };
  float s8[8], q8[8], bnm8[8], bnr8[8];
  #pragma unroll
  for (int e = 0; e < 8; ++e) { s8[e] = 0.f; q8[e] = 0.f; }
  if (bn_ps && bnb_x) {
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      if constexpr (PF > 0) {
        bnm8[e] = pf_bnm[e];
        bnr8[e] = pf_bnr[e];
      } else {
        int j = j_base + e;
        bnm8[e] = (j < K) ? bnb_mean[j] : 0.f;
        bnr8[e] = (j < K) ? bnb_rstd[j] : 0.f;
      }
    }
  }
  #pragma unroll
  for (int it = 0; it < WM / RPI; ++it) {
    const int row = it * RPI + e_row;
    const long m = m_base + row;
    if constexpr (PF > 0) {
      if (it + PFD < NIT) pf_issue(it + PFD);
    }
    uint4 val;
    float vf[F32B ? 8 : 1];
    if constexpr (F32B) {
      constexpr int WNF = WN + 4;   // fp32 row pitch: half a region fits
      constexpr int HIT = NIT / 2;  // iterations per half of WM/2 rows
      static_assert((WM / 2) * WNF * 4 <= WM * WNP * 2, "fp32 half fits");
      float* lF = reinterpret_cast<float*>(lC);
      if (it % HIT == 0) {
        #pragma unroll
        for (int mi = 0; mi < MF / 2; ++mi)
          #pragma unroll
          for (int ni = 0; ni < NF; ++ni)
            #pragma unroll
            for (int q = 0; q < 4; ++q)
              lF[(mi * 16 + d_row0 + q) * WNF + ni * 16 + d_col] =
                  acc[(it / HIT) * (MF / 2) + mi][ni][q];
      }
      const float* src = lF + (row - (it / HIT) * (WM / 2)) * WNF + e_ch * 8;
      const float4 lo = *reinterpret_cast<const float4*>(src);
      const float4 hi = *reinterpret_cast<const float4*>(src + 4);
      vf[0] = lo.x; vf[1] = lo.y; vf[2] = lo.z; vf[3] = lo.w;
      vf[4] = hi.x; vf[5] = hi.y; vf[6] = hi.z; vf[7] = hi.w;
    } else {
      val = *reinterpret_cast<const uint4*>(lC + row * WNP + e_ch * 8);
    }
    if constexpr (PF > 0) {
      // One drain once the last group is out and this iteration's LDS
      // traffic is issued (vmcnt(0); expcnt, lgkmcnt left alone). The
      // groups sit behind lane predicates, so without it the compiler
      // cannot know they have landed on every path and puts a vmcnt(0) —
      // which also waits for the previous iteration's store — in front of
      // each iteration.
      if (it == (NIT - PFD > 0 ? NIT - PFD - 1 : 0))
        __builtin_amdgcn_s_waitcnt(0x0F70);
    }
    if (m < M) {
      const long orow = out_row(m);
      if (j_base + 8 <= K) {
        if constexpr (F32B) {
          // early add, coalesced: fp32 accumulator + (masked) acc chunk,
          // one rounding — the arithmetic of the gather it replaces
          uint4 a = pf_a[it];
          unsigned mb = 0xffu;
          if constexpr (MASKED) mb = pf_am[it];
          const unsigned* aw = &a.x;
          unsigned* vw = &val.x;
          #pragma unroll
          for (int d = 0; d < 4; ++d) {
            float alo = b2f((bf16_t)(aw[d] & 0xffff));
            float ahi = b2f((bf16_t)(aw[d] >> 16));
            if (!((mb >> (2 * d)) & 1)) alo = 0.f;
            if (!((mb >> (2 * d + 1)) & 1)) ahi = 0.f;
            vw[d] = (unsigned)f2b(vf[2 * d] + alo) |
                    ((unsigned)f2b(vf[2 * d + 1] + ahi) << 16);
          }
          // From here on val is to the compiler what the LDS read is in the
          // other instantiations: an opaque bf16 chunk. Without this the
          // fast-math reassociation of the dgamma product below sees
          // through to the fp32 sum and picks another multiplication order
          // (measured: the partials then differ in the last bit).
          asm volatile("" : "+v"(val.x), "+v"(val.y), "+v"(val.z), "+v"(val.w));
          *reinterpret_cast<uint4*>(y + orow * K + j_base) = val;
        } else if (!MASKED && ep_scale) {
          uint4 a{0, 0, 0, 0};
          if (accp)
            a = *reinterpret_cast<const uint4*>(accp + orow * K + j_base);
          uint4 o;
          unsigned* ow = &o.x;
          const unsigned* vw = &val.x;
          const unsigned* aw = &a.x;
          #pragma unroll
          for (int d = 0; d < 4; ++d) {
            float alo = accp ? b2f((bf16_t)(aw[d] & 0xffff)) : 0.f;
            float ahi = accp ? b2f((bf16_t)(aw[d] >> 16)) : 0.f;
            bf16_t lo = ep_apply((bf16_t)(vw[d] & 0xffff), 2 * d, alo);
            bf16_t hi = ep_apply((bf16_t)(vw[d] >> 16), 2 * d + 1, ahi);
            ow[d] = (unsigned)lo | ((unsigned)hi << 16);
          }
          *reinterpret_cast<uint4*>(y + orow * K + j_base) = o;
        } else if (accp && !acc_early) {
          // accumulate: coalesced uint4 read of the add-input at the same
          // address, pairwise bf16 add in fp32 (matches the engine's
          // bf16+bf16 add numerics)
          uint4 a;
          if constexpr (PF > 0)
            a = pf_a[it];
          else
            a = *reinterpret_cast<const uint4*>(accp + orow * K + j_base);
          if constexpr (MASKED) {
            // one byte covers this 8-channel chunk; a cleared bit turns
            // its bf16 half into +0.0
            unsigned mb;
            if constexpr (PF > 0)
              mb = pf_am[it];
            else
              mb = acc_mask[(orow * K + j_base) >> 3];
            auto keep = [&](int e) -> unsigned {
              return (((mb >> e) & 1) ? 0xffffu : 0u) |
                     (((mb >> (e + 1)) & 1) ? 0xffff0000u : 0u);
            };
            a.x &= keep(0);
            a.y &= keep(2);
            a.z &= keep(4);
            a.w &= keep(6);
          }
          auto addpair =[&](unsigned v, unsigned aw) -> unsigned {
            bf16_t lo = f2b(b2f((bf16_t)(v & 0xffff)) + b2f((bf16_t)(aw & 0xffff)));
            bf16_t hi = f2b(b2f((bf16_t)(v >> 16)) + b2f((bf16_t)(aw >> 16)));
            return (unsigned)lo | ((unsigned)hi << 16);
          };
          val.x = addpair(val.x, a.x);
          val.y = addpair(val.y, a.y);
          val.z = addpair(val.z, a.z);
          val.w = addpair(val.w, a.w);
          *reinterpret_cast<uint4*>(y + orow * K + j_base) = val;
        } else {
          *reinterpret_cast<uint4*>(y + orow * K + j_base) = val;
        }
        if (bn_ps) {
          if (bnb_x) {
            // BN-BWD partials: masked dy and dy*xhat (j_base is 8-aligned
            // so the mask byte covers exactly this chunk)
            unsigned mb;
            uint4 xv;
            if constexpr (PF > 0) {
              mb = pf_xm[it];
              xv = pf_x[it];
            } else {
              mb = bnb_mask ? bnb_mask[(orow * K + j_base) >> 3] : 0xffu;
              xv = *reinterpret_cast<const uint4*>(bnb_x + orow * K + j_base);
            }
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
              unsigned wd = (e < 2) ? val.x : (e < 4) ? val.y : (e < 6) ? val.z : val.w;
              unsigned xw = (e < 2) ? xv.x : (e < 4) ? xv.y : (e < 6) ? xv.z : xv.w;
              if ((mb >> e) & 1) {
                float f = b2f((bf16_t)(wd >> ((e & 1) * 16)));
                float xf = b2f((bf16_t)(xw >> ((e & 1) * 16)));
                s8[e] += f;
                q8[e] += f * (xf - bnm8[e]) * bnr8[e];
              }
            }
          } else {
            // fused fwd BN statistics
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
              unsigned wd = (e < 2) ? val.x : (e < 4) ? val.y : (e < 6) ? val.z : val.w;
              float f = b2f((bf16_t)(wd >> ((e & 1) * 16)));
              s8[e] += f;
              q8[e] += f * f;
            }
          }
        }
      } else if constexpr (PF == 0) {
        // (the PF instantiations run only where K % 8 == 0 — the launcher
        // sees to it — so a chunk is whole or dead and this scalar tail,
        // whose loads would put a wait into every iteration, is left out)
        // static component extraction (a reinterpret pointer into `val`
        // forces the register to scratch — rule 20)
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (j_base + e < K) {
            unsigned wd = (e < 2) ? val.x : (e < 4) ? val.y : (e < 6) ? val.z : val.w;
            bf16_t ov = (bf16_t)(wd >> ((e & 1) * 16));
            if (!MASKED && ep_scale) {
              float av = accp ? b2f(accp[orow * K + j_base + e]) : 0.f;
              ov = ep_apply(ov, e, av);
            } else if (accp && !acc_early) {
              float av = b2f(accp[orow * K + j_base + e]);
              if constexpr (MASKED) {
                if (!((acc_mask[(orow * K + j_base) >> 3] >> e) & 1)) av = 0.f;
              }
              ov = f2b(b2f(ov) + av);
            }
            y[orow * K + j_base + e] = ov;
            if (bn_ps) {
              float f = b2f(ov);
              if (bnb_x) {
                bool on = !bnb_mask ||
                          ((bnb_mask[(orow * K + j_base) >> 3] >> e) & 1);
                if (on) {
                  s8[e] += f;
                  q8[e] += f * (b2f(bnb_x[orow * K + j_base + e]) - bnm8[e]) *
                           bnr8[e];
                }
              } else {
                s8[e] += f;
                q8[e] += f * f;
              }
            }
          }
        }
      }
    }
  }
  if (bn_ps) {
    // lanes sharing e_ch (= lane % CPL) hold disjoint row groups of the
    // same 8 channels: xor-reduce over the row bits, lanes < CPL write
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      for (int msk = CPL; msk < 64; msk <<= 1) {
        s8[e] += __shfl_xor(s8[e], msk, 64);
        q8[e] += __shfl_xor(q8[e], msk, 64);
      }
    }
    if (lane < CPL) {
      const long prow_ = tile_m * 2 + wr;  // WVM = BM/WM = 2
      #pragma unroll
      for (int e = 0; e < 8; ++e) {
        int j = j_base + e;
        if (j < K) {
          bn_ps[prow_ * K + j] = s8[e];
          bn_pq[prow_ * K + j] = q8[e];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Wide-tile pipelined variant: BM=256, 8 waves (512 thr), THREE LDS K-tile
// buffers, counted-vmcnt + raw-barrier span (cdna guide §5 T3/T4: a glds
// stays in flight ACROSS the barrier; `__syncthreads()` would emit a
// vmcnt(0) drain — the ~20% stall of the 2-buffer structure at 1 block/CU),
// s_setprio(1) around the MFMA cluster (T5: pays on phase-split schedules).
// Used on long-K-loop shapes (3x3 layers, deep 1x1s) where the 128² 2-buffer
// kernel measured 540-720 TF/s ≈ 22-29% of peak (profiles/conv_mfma_pmc.md).
//
// Per K-tile glds count = (BM + BN) / 64 (one 8-KiB piece per 64 LDS rows,
// each piece = 1 glds per wave); the gate before computing tile t+1 is
// s_waitcnt vmcnt(GLDS) — tile t+2's loads keep flying across the barrier.
// ---------------------------------------------------------------------------
template <int BM, int BN, int NB>  // NB = LDS K-tile buffers (3 = span
                                   // with one tile in flight; 2 = stage
                                   // hidden behind the current compute)
__global__ __launch_bounds__(512, 1) void k_conv_igemm_wide(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ y, const bf16_t* __restrict__ zpage,
    int N, int H, int W_, int C, int K, int Ho, int Wo,
    int R, int S, int stride, int pad, int nwg_swz,
    int oH, int oW, int oS,
    unsigned long long magic_wo, unsigned shift_wo,
    unsigned long long magic_ho, unsigned shift_ho,
    const bf16_t* __restrict__ accp,
    float* __restrict__ bn_ps, float* __restrict__ bn_pq,
    const bf16_t* __restrict__ bnb_x,
    const unsigned char* __restrict__ bnb_mask,
    const float* __restrict__ bnb_mean,
    const float* __restrict__ bnb_rstd) {
  constexpr int BK = 64;
  constexpr int WAVES = 8;            // 4 (M) x 2 (N)
  constexpr int WM = BM / 4, WN = BN / 2;
  constexpr int MF = WM / 16, NF = WN / 16;
  constexpr int AP = BM / 64;         // 1-KiB A pieces per wave (8 rows each)
  constexpr int BP = BN / 64;
  constexpr int GLDS = AP + BP;       // glds per wave per K-tile
  constexpr int AHEAD = NB - 1;       // tiles staged ahead of the compute
  constexpr int BUF = (BM + BN) * BK; // bf16 elements per K-tile buffer
  __shared__ __attribute__((aligned(16))) bf16_t smem[NB * BUF];

  const long M = (long)N * Ho * Wo;
  const int tiles_n = (K + BN - 1) / BN;

  int wg = blockIdx.x;
  {
    int nwg = nwg_swz;
    int q = nwg >> 3, rm = nwg & 7;
    int xcd = wg & 7, i = wg >> 3;
    wg = (xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + i;
  }
  const int tile_n = wg % tiles_n;
  const long tile_m = wg / tiles_n;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  const int prow = lane >> 3;
  const int pcol8 = lane & 7;
  long a_m[AP];
  int a_hb[AP], a_wb[AP];
  const bf16_t* a_base[AP];
  #pragma unroll
  for (int p = 0; p < AP; ++p) {
    int row = (wave * AP + p) * 8 + prow;
    long m = tile_m * BM + row;
    a_m[p] = m;
    if (m < M) {
      unsigned mu = (unsigned)m;
      unsigned q1 = mdiv(mu, magic_wo, shift_wo);
      int wo = (int)(mu - q1 * (unsigned)Wo);
      unsigned n_u = mdiv(q1, magic_ho, shift_ho);
      int ho = (int)(q1 - n_u * (unsigned)Ho);
      int n = (int)n_u;
      a_hb[p] = ho * stride - pad;
      a_wb[p] = wo * stride - pad;
      a_base[p] = x + (((long)n * H + a_hb[p]) * W_ + a_wb[p]) * C +
                  (pcol8 ^ ((((wave * AP + p) & 1) << 2) | (prow >> 1))) * 8;
    } else {
      a_hb[p] = -100000;
      a_wb[p] = -100000;
      a_base[p] = zpage;
    }
  }
  const long KRS = (long)R * S * C;
  const bf16_t* b_base[BP];
  bool b_ok[BP];
  #pragma unroll
  for (int p = 0; p < BP; ++p) {
    int row = (wave * BP + p) * 8 + prow;
    int j = tile_n * BN + row;
    b_ok[p] = j < K;
    b_base[p] = b_ok[p]
        ? (w + (long)j * KRS +
           (pcol8 ^ ((((wave * BP + p) & 1) << 2) | (prow >> 1))) * 8)
        : zpage;
  }

  // staging split into two interleavable halves: glds issue slots are
  // expensive when burst together (60-185 cyc each in a crowded phase);
  // spreading them between the two k-half MFMA clusters hides the issue
  // cost under the matrix pipe (the 8-phase-template idea, coarse form)
  auto stage_half = [&](int buf, int r, int s, int ck, int half) {
    bf16_t* lA = smem + buf * BUF;
    bf16_t* lB = lA + BM * BK;
    const long aoff = ((long)r * W_ + s) * C + ck;
    #pragma unroll
    for (int p = 0; p < AP; ++p) {
      if ((p & 1) != half) continue;
      int h = a_hb[p] + r, ww = a_wb[p] + s;
      bool ok = (a_m[p] < M) & (h >= 0) & (h < H) & (ww >= 0) & (ww < W_);
      const bf16_t* src = ok ? (a_base[p] + aoff) : zpage;
      __builtin_amdgcn_global_load_lds(
          (const GLOBAL_AS void*)src,
          (LDS_AS void*)(lA + (wave * AP + p) * 512), 16, 0, 0);
    }
    const long boff = ((long)r * S + s) * C + ck;
    #pragma unroll
    for (int p = 0; p < BP; ++p) {
      if ((p & 1) != half) continue;
      const bf16_t* src = b_ok[p] ? (b_base[p] + boff) : zpage;
      __builtin_amdgcn_global_load_lds(
          (const GLOBAL_AS void*)src,
          (LDS_AS void*)(lB + (wave * BP + p) * 512), 16, 0, 0);
    }
  };

  f32x4_v acc[MF][NF];
  #pragma unroll
  for (int mi = 0; mi < MF; ++mi)
    #pragma unroll
    for (int ni = 0; ni < NF; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

  const int fr_row = lane & 15;
  const int fr_c8 = lane >> 4;

  const int csteps = C / BK;
  const int T = R * S * csteps;
  int r2 = 0, s2 = 0, ck2 = 0;
  auto advance = [&]() {
    ck2 += BK;
    if (ck2 >= C) {
      ck2 = 0;
      if (++s2 >= S) { s2 = 0; ++r2; }
    }
  };

  // prologue: tiles 0..AHEAD-1 issued; gate tile 0 landed
  stage_half(0, r2, s2, ck2, 0);
  stage_half(0, r2, s2, ck2, 1);
  advance();
  if (AHEAD > 1 && T > 1) {
    stage_half(1, r2, s2, ck2, 0);
    stage_half(1, r2, s2, ck2, 1);
    advance();
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GLDS) : "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();

  for (int t = 0; t < T; ++t) {
    const bool more = (t + AHEAD) < T;
    const int nbuf = (t + AHEAD) % NB, nr = r2, ns = s2, nck = ck2;
    if (more) advance();
    const bf16_t* lA = smem + (t % NB) * BUF;
    const bf16_t* lB = lA + BM * BK;
    #pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      if (more) stage_half(nbuf, nr, ns, nck, kh);
      bf16x8_v fa[MF], fb[NF];
      #pragma unroll
      for (int mi = 0; mi < MF; ++mi) {
        int row = wr * WM + mi * 16 + fr_row;
        int c8 = (kh * 4 + fr_c8) ^ ((row >> 1) & 7);
        fa[mi] = *reinterpret_cast<const bf16x8_v*>(lA + row * BK + c8 * 8);
      }
      #pragma unroll
      for (int ni = 0; ni < NF; ++ni) {
        int row = wc * WN + ni * 16 + fr_row;
        int c8 = (kh * 4 + fr_c8) ^ ((row >> 1) & 7);
        fb[ni] = *reinterpret_cast<const bf16x8_v*>(lB + row * BK + c8 * 8);
      }
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int mi = 0; mi < MF; ++mi)
        #pragma unroll
        for (int ni = 0; ni < NF; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    if (t + 1 < T) {
      // tile t+1 must have landed before any wave reads it; with NB=3 the
      // newest tile's GLDS loads stay in flight across the barrier
      if (AHEAD > 1 && more)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GLDS) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }

  // direct-store epilogue (long K-loop shapes: store tail amortized)
  const int d_col = lane & 15;
  const int d_row0 = (lane >> 4) * 4;
  auto out_row = [&](long m) -> long {
    if (oS == 1) return m;
    unsigned mu = (unsigned)m;
    unsigned q1 = mdiv(mu, magic_wo, shift_wo);
    int wo = (int)(mu - q1 * (unsigned)Wo);
    unsigned n_u = mdiv(q1, magic_ho, shift_ho);
    int ho = (int)(q1 - n_u * (unsigned)Ho);
    return ((long)(int)n_u * oH + (long)ho * oS) * oW + (long)wo * oS;
  };
  auto b2f = [](bf16_t u) -> float {
    union { unsigned i; float f; } cvt;
    cvt.i = (unsigned)u << 16;
    return cvt.f;
  };
  // accp hoisted OUT of the unrolled loops: a per-element runtime select
  // around a load makes hipcc branch + wait vmcnt(0) per element
  auto epilogue = [&](auto has_acc) {
    #pragma unroll
    for (int mi = 0; mi < MF; ++mi) {
      #pragma unroll
      for (int ni = 0; ni < NF; ++ni) {
        int j = tile_n * BN + wc * WN + ni * 16 + d_col;
        if (j >= K) continue;
        #pragma unroll
        for (int q = 0; q < 4; ++q) {
          long m = tile_m * BM + wr * WM + mi * 16 + d_row0 + q;
          if (m < M) {
            long oi = out_row(m) * K + j;
            float v = acc[mi][ni][q];
            if constexpr (decltype(has_acc)::value) v += b2f(accp[oi]);
            y[oi] = f2b(v);
          }
        }
      }
    }
  };
  if (accp)
    epilogue(std::true_type{});
  else
    epilogue(std::false_type{});
  // NOTE: the wide tiles are never routed for fused BN stats / bnb
  // (pick_tile excludes them) — the partials epilogue is omitted here to
  // keep the 256x256 instantiation under the register cap (with it the
  // kernel spilled 528 B/lane).
  (void)bn_ps; (void)bn_pq; (void)bnb_x; (void)bnb_mask;
  (void)bnb_mean; (void)bnb_rstd;
}

// ---------------------------------------------------------------------------
// launcher: picks the tile instantiation by shape
// ---------------------------------------------------------------------------
struct TilePick {
  int bm, bn, bufs, wvm;
  bool epi_lds, wide, m32;
};

// One tile decision for launcher + nparts query (must stay in sync by
// construction). want_stats forces the 16x16 direct epilogue (the only
// ones carrying the bn-partials code). want_mask (masked accumulate) lives
// in the same two epilogues: never the wide or the 32x32 route.
static TilePick pick_tile(long M, int K, int C, int T, bool want_stats,
                          bool want_bnb = false, bool want_ep = false,
                          bool want_mask = false) {
  int mfma_pref, wide_pref;
  {
    const char* e = getenv("DDLW_CONV_MFMA");
    mfma_pref = (e && e[0] == '3') ? 32 : 16;
    const char* e2 = getenv("DDLW_CONV_WIDE");
    wide_pref = e2 ? (e2[0] == '0' ? 0 : 1) : -1;  // -1 = auto
  }
  TilePick p{};
  p.m32 = (mfma_pref == 32) && !want_stats && !want_bnb && !want_mask;
  // measured (bench/tools/wide_check.py + whole-model A/B on MI355X): the
  // 256x256 2-buf wide kernel wins +20-28% on its isolated shapes
  // (K >= 256, T >= 9, >= 150 blocks) but the full ResNet-50 step runs
  // ~1% SLOWER with it auto-routed (repeated A/B; DVFS/L2-context effect:
  // the denser kernels depress the whole-step clock by more than their
  // isolated win). Auto routing is therefore OFF — a documented negative
  // result; DDLW_CONV_WIDE=1 forces it for probes.
  const bool wide_auto = false;
  if (!want_bnb && !want_stats && !want_ep && !want_mask &&
      ((wide_pref == 1 && K >= 128 && T >= 4) || (wide_pref == -1 && wide_auto))) {
    p.wide = true;
    p.bm = 256;
    p.bn = (K >= 256) ? 256 : 128;
    p.bufs = (p.bn == 256) ? 2 : 3;
    p.wvm = 4;
    return p;
  }
  p.bm = 128;
  p.wvm = 2;
  // (A BN=256 single-buffer tile for the T==1 K>=256 1x1 layers — halving
  // B re-reads and block count — measured 111 vs 195 TF and -2.8% on the
  // whole step: 128 acc VGPRs + 132 AGPRs force 1 block/CU and the
  // latency-bound single-K-step kernel lives on block-level overlap.
  // Removed; the 128x128 BUFS=1 tile at 4 blocks/CU is ~73% of its
  // memory roofline already.)
  p.bn = (K >= 128) ? 128 : (K >= 64 ? 64 : 32);
  // bnb (fused BN-backward reduce) must use the LDS-bounce epilogue on
  // EVERY shape: the direct epilogue's per-element stride-K x loads are
  // uncoalesced scalar L2 round trips (measured -7% whole-model)
  p.epi_lds = (T <= 4) || want_bnb;
  p.bufs = (T == 1) ? 1 : 2;
  return p;
}

// DDLW_EPI_PREFETCH: 0 -> off, anything else or unset -> on
static bool epi_prefetch_lever() {
  const char* e = getenv("DDLW_EPI_PREFETCH");
  return !(e && e[0] == '0');
}

DDLW_EXPORT long ddlw_conv_fwd_nparts(int N, int C, int K, int Ho, int Wo,
                                      int R, int S, int bnb) {
  long M = (long)N * Ho * Wo;
  const int T = R * S * (C / 64);
  TilePick p = pick_tile(M, K, C, T, true, bnb != 0);
  return cdiv(M, p.bm) * p.wvm;
}

// The one conv-forward entry point; a null pointer switches that fusion off.
//   acc           y += acc (residual-join gradient add in conv1's dgrad)
//   acc_mask      with acc: y += (bit ? acc : 0), one byte per 8 output
//                 channels in k_bn_apply's relu-mask layout, so the join reads
//                 dy and bn3's mask instead of a masked copy of dy
//   bn_ps/bn_pq   fused BN statistics: per-(tile_m, wave-row) sum/sumsq rows
//   bnb_*         dgrad + fused BN-backward reduce: bn_ps/bn_pq receive the
//                 (dbeta, dgamma) partials against (bnb_x, mask, mean, rstd),
//                 so k_bn_bwd_reduce never re-reads dy
//   ep_*          eval-mode BN fold: y = relu?(conv*scale[k] + bias[k] [+ acc])
//   oH/oW/oS      output scatter geometry (Ho/Wo/1 for a plain conv)
DDLW_EXPORT int ddlw_conv_fwd_igemm(const void* x, const void* w, void* y,
                                    const void* zpage, const void* acc,
                                    const void* acc_mask,
                                    void* bn_ps, void* bn_pq,
                                    const void* bnb_x, const void* bnb_mask,
                                    const void* bnb_mean, const void* bnb_rstd,
                                    const void* ep_scale, const void* ep_bias,
                                    int ep_relu,
                                    int N, int H, int W_, int C, int K,
                                    int Ho, int Wo, int R, int S, int stride,
                                    int pad, int oH, int oW, int oS,
                                    void* stream) {
  if (C % 64 != 0) {
    ddlw_set_error("conv_fwd_igemm: C must be a multiple of 64");
    return 2;
  }
  if (acc_mask && (!acc || ep_scale || K % 8 != 0))
    return ddlw_fail("conv_fwd_igemm",
                     "acc_mask needs acc, no ep_scale and K a multiple of 8");
  long M = (long)N * Ho * Wo;
  if (M >= (1ll << 31)) {
    ddlw_set_error("conv_fwd_igemm: M >= 2^31 unsupported");
    return 2;
  }
  unsigned long long mg_wo, mg_ho;
  unsigned sh_wo, sh_ho;
  make_magic((unsigned)Wo, &mg_wo, &sh_wo);
  make_magic((unsigned)Ho, &mg_ho, &sh_ho);
  const int T = R * S * (C / 64);
  hipStream_t st = (hipStream_t)stream;
  const bool want_stats = bn_ps != nullptr;
  const bool want_bnb = bnb_x != nullptr;
  // the eval-BN fold epilogue lives only in the base kernel
  const bool want_ep = ep_scale != nullptr;
  TilePick p = pick_tile(M, K, C, T, want_stats, want_bnb, want_ep,
                         acc_mask != nullptr);
  if (p.wide) {
    long grid = cdiv(M, 256) * cdiv(K, p.bn);
#define WIDE_LAUNCH(BN_, NB_)                                                  \
    hipLaunchKernelGGL((k_conv_igemm_wide<256, BN_, NB_>), dim3((int)grid),    \
                       dim3(512), 0, st, (const bf16_t*)x, (const bf16_t*)w,   \
                       (bf16_t*)y, (const bf16_t*)zpage, N, H, W_, C, K, Ho,   \
                       Wo, R, S, stride, pad, (int)grid, oH, oW, oS, mg_wo,    \
                       sh_wo, mg_ho, sh_ho, (const bf16_t*)acc,                \
                       (float*)bn_ps, (float*)bn_pq, (const bf16_t*)bnb_x,     \
                       (const unsigned char*)bnb_mask,                         \
                       (const float*)bnb_mean, (const float*)bnb_rstd)
    if (p.bn == 256)
      WIDE_LAUNCH(256, 2);
    else
      WIDE_LAUNCH(128, 3);
#undef WIDE_LAUNCH
    DDLW_CHECK_LAUNCH();
  }
  // Bounce epilogue that carries acc or bnb: side reads prefetched (the PF
  // instantiations), same bits. DDLW_EPI_PREFETCH=0 restores the in-order
  // instantiations below; read per call. They have no scalar tail for a
  // partial 8-channel chunk, so K % 8 != 0 stays in order too, and so does
  // the BN = 32 tile (K < 64: no layer of the models here, not measured).
  // Depth 7 of the 8 store-loop
  // iterations (the 8th group goes out in iteration 0; narrower tiles have
  // 4 or 2 iterations, all in flight): the most the 128x128 tiles hold at
  // 2 waves/SIMD (188 VGPR + 64..68 AGPR). The two-buffer tiles sit at 2
  // waves by LDS anyway; the one-buffer tile gives up its third wave for it
  // (one iteration ahead already takes 108 + 68 registers, over the 168 that
  // three waves leave).
  const bool early = acc && want_bnb && T > 4;
  // The unmasked early add stays in order as well: its PF instantiation is
  // 1.9x faster (285 -> 148 us at 14x14 512 -> 1024, B = 256) but the
  // compiler multiplies the dgamma term f * (x - mean) * rstd in another
  // order there (fast-math), and the partials differ in the last bit.
  if (epi_prefetch_lever() && (acc || want_bnb) && !want_ep && !p.m32 &&
      K % 8 == 0 && p.bn >= 64 && (p.epi_lds || early) &&
      !(early && !acc_mask)) {
    with_int<128, 64>(p.bn, [&](auto BN) {
      with_bool(acc_mask != nullptr, [&](auto MSK) {
        long grid = cdiv(M, 128) * cdiv(K, decltype(BN)::value);
#define PF_LAUNCH(BUFS_, EARLY_)                                               \
        hipLaunchKernelGGL(                                                    \
            (k_conv_fwd_igemm<128, decltype(BN)::value, true, BUFS_, false,    \
                              EARLY_, decltype(MSK)::value, 7>),               \
            dim3((int)grid), dim3(256), 0, st, (const bf16_t*)x,               \
            (const bf16_t*)w, (bf16_t*)y, (const bf16_t*)zpage, N, H, W_, C,   \
            K, Ho, Wo, R, S, stride, pad, (int)grid, oH, oW, oS, mg_wo, sh_wo, \
            mg_ho, sh_ho, (const bf16_t*)acc, (const unsigned char*)acc_mask,  \
            (float*)bn_ps, (float*)bn_pq, (const bf16_t*)bnb_x,                \
            (const unsigned char*)bnb_mask, (const float*)bnb_mean,            \
            (const float*)bnb_rstd, nullptr, nullptr, 0)
        if constexpr (decltype(MSK)::value) {
          if (early) {
            PF_LAUNCH(2, true);
            return;
          }
        }
        if (p.bufs == 2)
          PF_LAUNCH(2, false);
        else
          PF_LAUNCH(1, false);
#undef PF_LAUNCH
      });
    });
    DDLW_CHECK_LAUNCH();
  }
  if (early) {
    // acc + bnb on a shape whose own route is the direct epilogue: the
    // bounce epilogue with the early (fp32) accumulate, so dx is the same
    // with and without the reduce partials
    with_int<128, 64, 32>(p.bn, [&](auto BN) {
     with_bool(acc_mask != nullptr, [&](auto MSK) {
      long grid = cdiv(M, 128) * cdiv(K, decltype(BN)::value);
      hipLaunchKernelGGL(
          (k_conv_fwd_igemm<128, decltype(BN)::value, true, 2, false, true,
                            decltype(MSK)::value>),
          dim3((int)grid), dim3(256), 0, st, (const bf16_t*)x,
          (const bf16_t*)w, (bf16_t*)y, (const bf16_t*)zpage, N, H, W_, C, K,
          Ho, Wo, R, S, stride, pad, (int)grid, oH, oW, oS, mg_wo, sh_wo,
          mg_ho, sh_ho, (const bf16_t*)acc, (const unsigned char*)acc_mask,
          (float*)bn_ps, (float*)bn_pq, (const bf16_t*)bnb_x,
          (const unsigned char*)bnb_mask, (const float*)bnb_mean,
          (const float*)bnb_rstd, nullptr, nullptr, 0);
     });
    });
    DDLW_CHECK_LAUNCH();
  }
  if (acc_mask) {
    // masked accumulate: its own instantiations (16x16 MFMA, no ep fold)
    with_int<128, 64, 32>(p.bn, [&](auto BN) {
      with_bool(p.epi_lds, [&](auto EPI) {
        with_int<1, 2>(p.bufs, [&](auto BUFS) {
          long grid = cdiv(M, 128) * cdiv(K, decltype(BN)::value);
          hipLaunchKernelGGL(
              (k_conv_fwd_igemm<128, decltype(BN)::value, decltype(EPI)::value,
                                decltype(BUFS)::value, false, false, true>),
              dim3((int)grid), dim3(256), 0, st, (const bf16_t*)x,
              (const bf16_t*)w, (bf16_t*)y, (const bf16_t*)zpage, N, H, W_, C,
              K, Ho, Wo, R, S, stride, pad, (int)grid, oH, oW, oS, mg_wo,
              sh_wo, mg_ho, sh_ho, (const bf16_t*)acc,
              (const unsigned char*)acc_mask, (float*)bn_ps, (float*)bn_pq,
              (const bf16_t*)bnb_x, (const unsigned char*)bnb_mask,
              (const float*)bnb_mean, (const float*)bnb_rstd, nullptr, nullptr,
              0);
        });
      });
    });
    DDLW_CHECK_LAUNCH();
  }
  with_int<128, 64, 32>(p.bn, [&](auto BN) {
    with_bool(p.epi_lds, [&](auto EPI) {
      with_int<1, 2>(p.bufs, [&](auto BUFS) {
        with_bool(p.m32, [&](auto M32) {
          long grid = cdiv(M, 128) * cdiv(K, decltype(BN)::value);
          hipLaunchKernelGGL(
              (k_conv_fwd_igemm<128, decltype(BN)::value, decltype(EPI)::value,
                                decltype(BUFS)::value, decltype(M32)::value>),
              dim3((int)grid), dim3(256), 0, st, (const bf16_t*)x,
              (const bf16_t*)w, (bf16_t*)y, (const bf16_t*)zpage, N, H, W_, C,
              K, Ho, Wo, R, S, stride, pad, (int)grid, oH, oW, oS, mg_wo,
              sh_wo, mg_ho, sh_ho, (const bf16_t*)acc,
              (const unsigned char*)acc_mask, (float*)bn_ps,
              (float*)bn_pq, (const bf16_t*)bnb_x,
              (const unsigned char*)bnb_mask, (const float*)bnb_mean,
              (const float*)bnb_rstd, (const float*)ep_scale,
              (const float*)ep_bias, ep_relu);
        });
      });
    });
  });
  DDLW_CHECK_LAUNCH();
}

// merged-class stride-2 3x3 dgrad (even ih/iw): dx = scattered union of 4
// parity-class stride-1 convs of dy, one launch (grid.y = class).
DDLW_EXPORT int ddlw_conv_dgrad_s2m(const void* dy, const void* wcat, void* dx,
                                    const void* zpage, int N, int Ho, int Wo,
                                    int Kdy, int Cdx, int oh, int ow, int ih,
                                    int iw, const long* woffs,
                                    const long* yoffs, const int* crs,
                                    void* stream) {
  if (Kdy % 64 != 0) {
    ddlw_set_error("conv_dgrad_s2m: dy channels must be a multiple of 64");
    return 2;
  }
  long M = (long)N * oh * ow;
  if (M >= (1ll << 31)) {
    ddlw_set_error("conv_dgrad_s2m: M >= 2^31 unsupported");
    return 2;
  }
  unsigned long long mg_wo, mg_ho;
  unsigned sh_wo, sh_ho;
  make_magic((unsigned)ow, &mg_wo, &sh_wo);
  make_magic((unsigned)oh, &mg_ho, &sh_ho);
  S2Quad q;
  for (int i = 0; i < 4; ++i)
    q.c[i] = S2Class{woffs[i], yoffs[i], crs[2 * i], crs[2 * i + 1]};
  hipStream_t st = (hipStream_t)stream;
  int s2epi = 1;
  {
    const char* e = getenv("DDLW_S2_EPI");
    if (e && e[0] == '0') s2epi = 0;
  }
  with_bool(Cdx >= 128, [&](auto WIDE_N) {
    with_bool(s2epi != 0, [&](auto EPI) {
      constexpr int BN = decltype(WIDE_N)::value ? 128 : 64;
      long gx = cdiv(M, 128) * cdiv(Cdx, BN);
      hipLaunchKernelGGL(
          (k_conv_fwd_igemm<128, BN, decltype(EPI)::value, 2, false>),
          dim3((int)gx, 4), dim3(256), 0, st, (const bf16_t*)dy,
          (const bf16_t*)wcat, (bf16_t*)dx, (const bf16_t*)zpage, N, Ho, Wo,
          Kdy, Cdx, oh, ow, 2, 2, 1, 0, (int)gx, ih, iw, 2, mg_wo, sh_wo,
          mg_ho, sh_ho, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
          nullptr, nullptr, nullptr, nullptr, 0, 1, q);
    });
  });
  DDLW_CHECK_LAUNCH();
}
