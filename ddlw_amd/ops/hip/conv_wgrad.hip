// MFMA implicit-GEMM weight gradient (wrw) for CDNA4 (gfx950), NHWC bf16.
//
// Reference parity: the conv weight gradients TF computes behind model.fit
// for the trainable convs (SURVEY.md §2.4 K1-K3 "fwd+bwd for ResNet-50
// BASELINE configs"; the reference itself holds its base frozen,
// Part 1 .../02_model_training_single_node.py:167-169).
//
// dW[k][r][s][c] = sum_m dy[m][k] * x[m(r,s)][c]   (m = n*Ho*Wo rows)
//
// One GEMM per (r,s): dW_rs[K][C] = dy^T @ x_shifted, reduction over m.
// The m dimension is huge (up to N*Ho*Wo = 800k), so blocks split it
// (blockIdx.z) and write fp32 partial slabs reduced by a second kernel —
// deterministic, no atomics (same philosophy as the BN reductions).
//
// Both MFMA fragments are m-major per lane (kk = m), i.e. TRANSPOSED with
// respect to the natural [m][k] / [m][c] global layout. v2 avoids the
// 64-scalar-ds_write transpose of v1 entirely:
//   - tiles are staged with global_load_lds (async, 1 KiB per
//     wave-instruction) into a SUBTILED image: consecutive [4 rows][16 cols]
//     row-major blocks, even-m blocks before odd-m blocks within each 32-m
//     group — exactly the layout ds_read_b64_tr_b16 gathers conflict-free
//     (the attention-V recipe: lane l, elem j <- lds[(l&15) + j*16 +
//     (l>>4)*64]);
//   - fragments are read with TWO hardware transpose reads each (m 0-3 from
//     the even blocks, m 4-7 from the odd blocks), inline asm counted by an
//     explicit lgkmcnt(0) + sched_barrier(0) before the MFMAs
//     (cdna_hip_programming.md §5.4 rule 18, §5.7 form iii).
#include "igemm.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_v;
typedef __attribute__((ext_vector_type(4))) float f32x4_v;
typedef __attribute__((ext_vector_type(2))) unsigned tr64_t;

__device__ __forceinline__ unsigned lds_u32(const bf16_t* p) {
  return (unsigned)(unsigned long long)(const LDS_AS bf16_t*)p;
}

template <int BK, int BC, int WG_BM = 64>  // output tile: BK x BC (k x c);
                                           // WG_BM = m rows per k-step
__global__ __launch_bounds__(256) void k_conv_wgrad(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
    const bf16_t* __restrict__ zpage,
    float* __restrict__ slab,  // [SPLIT][K][RS*C]
    int N, int H, int W_, int C, int K, int Ho, int Wo,
    int R, int S, int stride, int pad,
    int split, long m_per_split,
    unsigned long long magic_wo, unsigned shift_wo,
    unsigned long long magic_ho, unsigned shift_ho) {
  constexpr int WK = BK / 2, WC = BC / 2;   // per-wave tile (2x2 wave grid)
  constexpr int KF = WK / 16, CF = WC / 16; // fragments
  constexpr int MG = WG_BM / 32;            // 32-m groups per k-step
  constexpr int PA = BK / 16 * MG;          // 1-KiB dy pieces (k16 x m32)
  constexpr int PB = BC / 16 * MG;          // 1-KiB x pieces
  constexpr int TILE = WG_BM * BK;          // elements per dy tile
  constexpr int BUF = WG_BM * (BK + BC);
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * BUF];

  const long M = (long)N * Ho * Wo;
  const int ctiles = (C + BC - 1) / BC;
  const int tile_k = blockIdx.x / ctiles;
  const int tile_c = blockIdx.x % ctiles;
  const int rs = blockIdx.y;
  const int r = rs / S, s = rs % S;
  const int sp = blockIdx.z;

  const long m0 = (long)sp * m_per_split;
  const long m1 = (m0 + m_per_split < M) ? (m0 + m_per_split) : M;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc2 = wave & 1;

  // ---- staging geometry: within a 1-KiB piece (one (k16, m32) segment of 8
  // [4][16] blocks, even-m blocks first), this lane's chunk is:
  //   pos = lane>>3, mr = (lane>>1)&3, half = lane&1
  //   mb  = pos<4 ? 2*pos : 2*(pos-4)+1   (block order inversion)
  const int s_pos = lane >> 3;
  const int s_mr = (lane >> 1) & 3;
  const int s_half = lane & 1;
  const int s_mb = (s_pos < 4) ? (2 * s_pos) : (2 * (s_pos - 4) + 1);
  const int s_mlocal = s_mb * 4 + s_mr;        // m within its 32-m group
  const int s_koff = s_half * 8;               // k offset within the k16

  // per-(m32) step state: global row pointers + validity for this lane
  const bf16_t* dyrow[MG];
  const bf16_t* xrow[MG];
  bool dv[MG], xv[MG];

  auto decompose = [&](long mbase) {
    #pragma unroll
    for (int g = 0; g < MG; ++g) {
      long m = mbase + g * 32 + s_mlocal;
      dv[g] = m < m1;
      dyrow[g] = dv[g] ? (dy + m * K) : zpage;
      bool ok = false;
      const bf16_t* xr = zpage;
      if (m < m1) {
        unsigned mu = (unsigned)m;
        unsigned q1 = mdiv(mu, magic_wo, shift_wo);
        int wo = (int)(mu - q1 * (unsigned)Wo);
        unsigned n_u = mdiv(q1, magic_ho, shift_ho);
        int ho = (int)(q1 - n_u * (unsigned)Ho);
        int hh = ho * stride - pad + r;
        int wwv = wo * stride - pad + s;
        ok = hh >= 0 && hh < H && wwv >= 0 && wwv < W_;
        if (ok) xr = x + (((long)(int)n_u * H + hh) * W_ + wwv) * C;
      }
      xv[g] = ok;
      xrow[g] = xr;
    }
  };

  // stage one WG_BM-row step into buffer `buf` (all glds; pieces round-robin
  // over waves; each piece is one (k16, m32) segment)
  auto stage = [&](int buf) {
    bf16_t* ldy = smem + buf * BUF;    // dy tile image
    bf16_t* lx = ldy + TILE;           // x tile image
    #pragma unroll
    for (int p = wave; p < PA; p += 4) {
      const int k16 = p / MG, g = p % MG;
      int kk = tile_k * BK + k16 * 16 + s_koff;
      const bf16_t* src = (dv[g] && kk < K) ? (dyrow[g] + kk) : zpage;
      __builtin_amdgcn_global_load_lds(
          (const GLOBAL_AS void*)src, (LDS_AS void*)(ldy + p * 512), 16, 0, 0);
    }
    #pragma unroll
    for (int p = wave; p < PB; p += 4) {
      const int c16 = p / MG, g = p % MG;
      int cc = tile_c * BC + c16 * 16 + s_koff;
      const bf16_t* src = (xv[g] && cc < C) ? (xrow[g] + cc) : zpage;
      __builtin_amdgcn_global_load_lds(
          (const GLOBAL_AS void*)src, (LDS_AS void*)(lx + p * 512), 16, 0, 0);
    }
  };

  f32x4_v acc[KF][CF];
  #pragma unroll
  for (int a = 0; a < KF; ++a)
    #pragma unroll
    for (int b = 0; b < CF; ++b) acc[a][b] = {0.f, 0.f, 0.f, 0.f};

  const long nsteps = (m1 - m0 + WG_BM - 1) / WG_BM;
  decompose(m0);
  stage(0);
  if (1 < nsteps) decompose(m0 + WG_BM);
  __syncthreads();

  int cur = 0;
  for (long t = 0; t < nsteps; ++t) {
    if (t + 1 < nsteps) {
      stage(cur ^ 1);
      if (t + 2 < nsteps) decompose(m0 + (t + 2) * WG_BM);
    }
    bf16_t* ldy = smem + cur * BUF;
    bf16_t* lx = ldy + TILE;
    #pragma unroll
    for (int mh = 0; mh < MG; ++mh) {  // 32-m groups of the WG_BM-m step
      // fragment loads: 2 hardware transpose reads per fragment
      tr64_t fk0[KF], fk1[KF], fc0[CF], fc1[CF];
      // per-lane address = base + lane*8 B: each 16-lane subgroup reads one
      // 128-B [4][16] block and the HW transpose hands lane l column l&15
      #pragma unroll
      for (int a = 0; a < KF; ++a) {
        const int k16 = (wr * WK) / 16 + a;
        unsigned addr = lds_u32(ldy + ((k16 * MG + mh) * 8) * 64) + lane * 8;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fk0[a]) : "v"(addr));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:512"
                     : "=v"(fk1[a]) : "v"(addr));
      }
      #pragma unroll
      for (int b = 0; b < CF; ++b) {
        const int c16 = (wc2 * WC) / 16 + b;
        unsigned addr = lds_u32(lx + ((c16 * MG + mh) * 8) * 64) + lane * 8;
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
          union { struct { tr64_t lo, hi; } p; bf16x8_v v; } fa, fb;
          fa.p.lo = fk0[a]; fa.p.hi = fk1[a];
          fb.p.lo = fc0[b]; fb.p.hi = fc1[b];
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              fa.v, fb.v, acc[a][b], 0, 0, 0);
        }
    }
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: D map col=lane&15 (c), row=(lane>>4)*4+q (k); fp32 slab write
  const long RSC = (long)R * S * C;
  float* out = slab + (long)sp * K * RSC;
  const int d_c = lane & 15;
  const int d_k0 = (lane >> 4) * 4;
  #pragma unroll
  for (int a = 0; a < KF; ++a) {
    #pragma unroll
    for (int b = 0; b < CF; ++b) {
      int c = tile_c * BC + wc2 * WC + b * 16 + d_c;
      if (c >= C) continue;
      #pragma unroll
      for (int q = 0; q < 4; ++q) {
        int k = tile_k * BK + wr * WK + a * 16 + d_k0 + q;
        if (k < K) out[(long)k * RSC + (long)rs * C + c] = acc[a][b][q];
      }
    }
  }
}

// reduce fp32 slabs -> bf16 dW (flat [K][RS*C] = channels_last weight grad).
// Block = 32 elements x 8 split-groups + LDS tree (a one-thread-per-element
// loop over up to 1024 strided partials is pure load latency — same lesson
// as the BN finalize kernels).
__global__ __launch_bounds__(256) void k_wgrad_reduce(
    const float* __restrict__ slab, bf16_t* __restrict__ dw,
    long elems, int split) {
  const int el = threadIdx.x & 31;
  const int pg = threadIdx.x >> 5;
  __shared__ float lds[8][32];
  for (long i0 = (long)blockIdx.x * 32; i0 < elems; i0 += (long)gridDim.x * 32) {
    const long i = i0 + el;
    float a = 0.f;
    if (i < elems)
      for (int p = pg; p < split; p += 8) a += slab[(long)p * elems + i];
    lds[pg][el] = a;
    __syncthreads();
    if (pg == 0 && i < elems) {
      #pragma unroll
      for (int g = 1; g < 8; ++g) a += lds[g][el];
      union { float f; unsigned u; } cvt;
      cvt.f = a;
      unsigned rb = 0x7FFF + ((cvt.u >> 16) & 1);
      dw[i] = (bf16_t)((cvt.u + rb) >> 16);
    }
    __syncthreads();
  }
}

DDLW_EXPORT int ddlw_conv_wgrad(const void* dy, const void* x, const void* zpage,
                                void* slab, void* dw, int N, int H, int W_,
                                int C, int K, int Ho, int Wo, int R, int S,
                                int stride, int pad, int split, void* stream) {
  if (C % 8 != 0 || K % 8 != 0) {
    ddlw_set_error("conv_wgrad: C and K must be multiples of 8");
    return 2;
  }
  long M = (long)N * Ho * Wo;
  if (M >= (1ll << 31)) {
    ddlw_set_error("conv_wgrad: M >= 2^31 unsupported");
    return 2;
  }
  unsigned long long mg_wo, mg_ho;
  unsigned sh_wo, sh_ho;
  make_magic((unsigned)Wo, &mg_wo, &sh_wo);
  make_magic((unsigned)Ho, &mg_ho, &sh_ho);
  long m_per_split = cdiv(M, split);
  hipStream_t st = (hipStream_t)stream;
#define WLAUNCH3(BK, BC, BM_)                                                 \
  do {                                                                        \
    dim3 grid((int)(cdiv(K, BK) * cdiv(C, BC)), R * S, split);                \
    hipLaunchKernelGGL((k_conv_wgrad<BK, BC, BM_>), grid, dim3(256), 0, st,   \
                       (const bf16_t*)dy, (const bf16_t*)x,                   \
                       (const bf16_t*)zpage, (float*)slab, N, H, W_, C, K,    \
                       Ho, Wo, R, S, stride, pad, split, m_per_split, mg_wo,  \
                       sh_wo, mg_ho, sh_ho);                                  \
  } while (0)
#define WLAUNCH(BK, BC)                                                       \
  do {                                                                        \
    dim3 grid((int)(cdiv(K, BK) * cdiv(C, BC)), R * S, split);                \
    hipLaunchKernelGGL((k_conv_wgrad<BK, BC>), grid, dim3(256), 0, st,        \
                       (const bf16_t*)dy, (const bf16_t*)x,                   \
                       (const bf16_t*)zpage, (float*)slab, N, H, W_, C, K,    \
                       Ho, Wo, R, S, stride, pad, split, m_per_split, mg_wo,  \
                       sh_wo, mg_ho, sh_ho);                                  \
  } while (0)
  // WG_BM=128 (a deeper 128-m k-step, WLAUNCH3(64,64,128)) measured EQUAL
  // OR SLOWER on every 64x64-tile route (110-234 vs 120-248 TF): the
  // small-tile wgrad is staging-bandwidth-bound (AI = 32 flops/B), not
  // barrier- or pipeline-depth-bound — documented negative result; the
  // instantiation is dropped (it also spilled 3 SGPRs).
  if (K >= 128 && C >= 128) WLAUNCH(128, 128);
  else if (C >= 128) WLAUNCH(64, 128);
  else if (K >= 128) WLAUNCH(128, 64);
  else WLAUNCH(64, 64);
#undef WLAUNCH
#undef WLAUNCH3
  DDLW_CHECK_LAUNCH_OR_RETURN();
  long elems = (long)K * R * S * C;
  long g = cdiv(elems, 32);
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((int)g), dim3(256), 0, st,
                     (const float*)slab, (bf16_t*)dw, elems, split);
  DDLW_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// Tap-fused 3x3 / stride 1 / pad 1 weight gradient.
//
// k_conv_wgrad runs one block per tap: nine blocks stage the same dy tile and
// nine shifted copies of x. Here one block owns a (64 k, 64 c) tile and a
// slice of output rows and produces all nine taps: 9 x (2x2) accumulator
// fragments per wave (144 registers). dy is staged once per step and its
// fragments are read from LDS once for the nine taps.
//
// Rows. Every output row is padded to PW m (PW = 8/16/32/64 >= Wo), so a 32-m
// MFMA group is made of whole rows and whole [4][16] blocks. The tap shift in
// s moves m by one, which a transpose read (four consecutive m out of one
// 128-B block) cannot address, so x is staged as three images per input row,
// one per s, from source addresses shifted by s-1. The shift in r is a whole
// row: the image of input row h serves output rows h-1, h and h+1, so the
// row images live in an LDS ring (slot = row & (NR-1)) and every input row is
// staged once per s.
//
// Image borders. Rows are numbered v = n*(H+1) + h + 1: one GAP row in front
// of every image. A gap row is staged from the zero page, in dy and in x, so
// the tap above row 0 and the tap below row H-1 read zeros and never the
// neighbouring image. Columns: m >= Wo of a padded row and taps left of
// column 0 / right of column W-1 are staged from the zero page as well. A
// slice [g0, g1) of output rows walks v from v(g0) to v(g1-1) in steps of RPS
// rows; x row v(g0)-1 (the halo above, a gap row when the slice starts an
// image) and x row v(g1-1)+1 are staged too, dy rows outside the slice and x
// rows past the lower halo come from the zero page.
//
// Row image: [c16][PW/4 blocks of [4 m][16 c]], within every unit of
// EB = min(PW/4, 8) blocks the even-m blocks before the odd-m blocks, so the
// two transpose reads of a fragment each take all their blocks of one row
// from one contiguous run. For PW < 32 the four 16-lane groups of a read
// gather from different rows (ring slots); the slot stride of PW = 8 is
// padded by 128 B so that two neighbouring rows fall on different banks.
template <int PW>
__global__ __launch_bounds__(256) void k_conv_wgrad3x3(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
    const bf16_t* __restrict__ zpage,
    float* __restrict__ slab,  // [SPLIT][K][9*C]
    int N, int H, int W_, int C, int K,
    int rows_q, int rows_rem,  // slice sizes: q rows, the first rem one more
    unsigned long long magic_h, unsigned shift_h) {
  constexpr int RPS = PW >= 32 ? 1 : 32 / PW;  // output rows per step
  constexpr int SM = RPS * PW;                 // m per step
  constexpr int MG = SM / 32;                  // 32-m groups per step
  constexpr int NR = 4 * RPS;                  // ring slots (>= 2*RPS + 2)
  constexpr int BPR = PW / 4;                  // blocks per row per c16
  constexpr int EB = BPR < 8 ? BPR : 8;        // blocks per even/odd unit
  constexpr int PP = PW / 8;                   // 1-KiB pieces per row image
  constexpr int ROWIMG = PW * 64;              // elements per (row, s) image
  constexpr int SLOT = 3 * ROWIMG + (PW == 8 ? 64 : 0);
  constexpr int DYIMG = SM * 64;
  constexpr unsigned ODD = EB / 2 * 128;       // bytes from even to odd block
  __shared__ __attribute__((aligned(16))) bf16_t smem[2 * DYIMG + NR * SLOT];
  bf16_t* const xring = smem + 2 * DYIMG;

  const int ctiles = C / 64;
  const int tile_k = blockIdx.x / ctiles;
  const int tile_c = blockIdx.x % ctiles;
  const int sp = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc2 = wave & 1;

  // slice [g0, g1) of the N*H output rows -> virtual rows [v0, v1)
  const int g0 = sp * rows_q + (sp < rows_rem ? sp : rows_rem);
  const int gl = g0 + rows_q + (sp < rows_rem ? 1 : 0) - 1;
  const int n0 = (int)mdiv((unsigned)g0, magic_h, shift_h);
  const int n1 = (int)mdiv((unsigned)gl, magic_h, shift_h);
  const int ho0 = g0 - n0 * H;
  const int L = (n1 - n0) * (H + 1) + (gl - n1 * H) - ho0 + 1;  // v1 - v0
  const int nsteps = (L + RPS - 1) / RPS;

  // staging lane geometry inside a 1-KiB piece (8 blocks of 8 16-B chunks)
  const int s_pos = lane >> 3;
  const int s_mr = (lane >> 1) & 3;
  const int s_koff = (lane & 1) * 8;

  // next row to stage, as (image, row + 1 within the image, row - (v0 - 1));
  // x starts at the halo row v0 - 1, dy at v0
  int xn = n0, xhp = ho0, xrel = 0;
  int dn = n0, dhp = ho0 + 1, drel = 1;

  auto stage_x = [&](auto count) {
    constexpr int COUNT = decltype(count)::value;
    constexpr int TOTAL = COUNT * 3 * PP;
    #pragma unroll
    for (int i = 0; i < (TOTAL + 3) / 4; ++i) {
      const int idx = i * 4 + wave;
      if (TOTAL % 4 != 0 && idx >= TOTAL) break;
      const int ric = idx / (3 * PP);
      const int s = (idx / PP) % 3;
      const int p = idx % PP;
      int n = xn, hp = xhp + ric;
      while (hp > H) { hp -= H + 1; ++n; }
      const int rel = xrel + ric;
      const bool rowok = hp >= 1 && rel <= L + 1 && n < N;
      // chunk position -> (c16, block of the row): even blocks come first
      const int P = p * 8 + s_pos;
      const int c16 = P / BPR;
      const int e = P % EB;
      const int b = e < EB / 2 ? 2 * e : 2 * (e - EB / 2) + 1;
      const int wo = ((P % BPR) / EB * EB + b) * 4 + s_mr;
      const int w = wo + s - 1;
      const bool ok = rowok && wo < W_ && w >= 0 && w < W_;
      const bf16_t* src =
          ok ? x + (((long)n * H + (hp - 1)) * W_ + w) * C + tile_c * 64 +
                   c16 * 16 + s_koff
             : zpage;
      bf16_t* dst = xring + (rel & (NR - 1)) * SLOT + s * ROWIMG + p * 512;
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)src,
                                       (LDS_AS void*)dst, 16, 0, 0);
    }
    xhp += COUNT;
    while (xhp > H) { xhp -= H + 1; ++xn; }
    xrel += COUNT;
  };

  auto stage_dy = [&](int buf) {
    bf16_t* ldy = smem + buf * DYIMG;
    #pragma unroll
    for (int i = 0; i < MG; ++i) {  // 4*MG pieces (k16, 32-m group)
      const int idx = i * 4 + wave;
      const int k16 = idx / MG, g = idx % MG;
      const int b = s_pos < 4 ? 2 * s_pos : 2 * (s_pos - 4) + 1;
      const int ms = g * 32 + b * 4 + s_mr;  // m within the step
      const int ri = ms / PW, wo = ms % PW;
      int n = dn, hp = dhp + ri;
      while (hp > H) { hp -= H + 1; ++n; }
      const bool ok = hp >= 1 && drel + ri <= L && wo < W_;
      const bf16_t* src =
          ok ? dy + (((long)n * H + (hp - 1)) * W_ + wo) * K + tile_k * 64 +
                   k16 * 16 + s_koff
             : zpage;
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)src,
                                       (LDS_AS void*)(ldy + idx * 512), 16, 0, 0);
    }
    dhp += RPS;
    while (dhp > H) { dhp -= H + 1; ++dn; }
    drel += RPS;
  };

  f32x4_v acc[9][2][2];
  #pragma unroll
  for (int t9 = 0; t9 < 9; ++t9)
    #pragma unroll
    for (int a = 0; a < 2; ++a)
      #pragma unroll
      for (int b = 0; b < 2; ++b) acc[t9][a][b] = {0.f, 0.f, 0.f, 0.f};

  // fragment-read lane geometry: 16-lane group q reads m = 8q .. 8q+7 of the
  // 32-m group, i.e. blocks 2q (first read) and 2q+1 (second) of padded row
  // (8q)/PW
  const int f_q = lane >> 4;
  const int f_ri = (f_q * 8) / PW;
  const int f_blk = ((f_q * 8) % PW) / 8;  // even block's place among evens
  const unsigned f_x = lds_u32(xring) + (unsigned)(wc2 * 2 * BPR + f_blk) * 128 +
                       (lane & 15) * 8;
  const unsigned f_dy = lds_u32(smem) + (unsigned)(wr * 2 * MG) * 1024 + lane * 8;

  stage_x(std::integral_constant<int, 2>{});
  stage_x(std::integral_constant<int, RPS>{});
  stage_dy(0);
  __syncthreads();

  int cur = 0;
  for (int t = 0; t < nsteps; ++t) {
    if (t + 1 < nsteps) {
      stage_dy(cur ^ 1);
      stage_x(std::integral_constant<int, RPS>{});
    }
    // ring slot of input row (out row + r - 1) for this lane's padded row
    unsigned xa[3];
    #pragma unroll
    for (int r = 0; r < 3; ++r)
      xa[r] = f_x + (unsigned)((t * RPS + f_ri + r) & (NR - 1)) * (SLOT * 2);
    const unsigned da = f_dy + (unsigned)cur * (DYIMG * 2);
    #pragma unroll
    for (int g = 0; g < MG; ++g) {
      tr64_t fk[2][2], fx[2][2][2];
      #pragma unroll
      for (int a = 0; a < 2; ++a) {
        const unsigned addr = da + (a * MG + g) * 1024;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(fk[a][0]) : "v"(addr));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:512"
                     : "=v"(fk[a][1]) : "v"(addr));
      }
      auto load_tap = [&](int tap, int fb) {
        const int r = tap / 3, s = tap % 3;
        #pragma unroll
        for (int b = 0; b < 2; ++b) {
          const unsigned addr =
              xa[r] + (unsigned)(s * ROWIMG * 2 + b * BPR * 128 + g * 1024);
          asm volatile("ds_read_b64_tr_b16 %0, %1"
                       : "=v"(fx[fb][b][0]) : "v"(addr));
          asm volatile("ds_read_b64_tr_b16 %0, %1"
                       : "=v"(fx[fb][b][1]) : "v"(addr + ODD));
        }
      };
      load_tap(0, 0);
      #pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        // the next tap's fragments load behind this tap's MFMAs
        if (tap + 1 < 9) load_tap(tap + 1, (tap + 1) & 1);
        #pragma unroll
        for (int a = 0; a < 2; ++a)
          #pragma unroll
          for (int b = 0; b < 2; ++b) {
            union { struct { tr64_t lo, hi; } p; bf16x8_v v; } fa, fb;
            fa.p.lo = fk[a][0]; fa.p.hi = fk[a][1];
            fb.p.lo = fx[tap & 1][b][0]; fb.p.hi = fx[tap & 1][b][1];
            acc[tap][a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                fa.v, fb.v, acc[tap][a][b], 0, 0, 0);
          }
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: D map col=lane&15 (c), row=(lane>>4)*4+q (k); fp32 slab write
  const long RSC = 9l * C;
  float* out = slab + (long)sp * K * RSC;
  const int c0 = tile_c * 64 + wc2 * 32 + (lane & 15);
  const int k0 = tile_k * 64 + wr * 32 + (lane >> 4) * 4;
  #pragma unroll
  for (int tap = 0; tap < 9; ++tap)
    #pragma unroll
    for (int a = 0; a < 2; ++a)
      #pragma unroll
      for (int b = 0; b < 2; ++b)
        #pragma unroll
        for (int q = 0; q < 4; ++q)
          out[(long)(k0 + a * 16 + q) * RSC + tap * C + c0 + b * 16] =
              acc[tap][a][b][q];
}

// 3x3 / stride 1 / pad 1 only (Ho = H, Wo = W_); `split` slices of whole
// output rows, sizes differing by at most one (conv_gemm.wgrad3x3_slices)
DDLW_EXPORT int ddlw_conv_wgrad3x3(const void* dy, const void* x,
                                   const void* zpage, void* slab, void* dw,
                                   int N, int H, int W_, int C, int K, int R,
                                   int S, int stride, int pad, int split,
                                   void* stream) {
  const char* who = "conv_wgrad3x3";
  if (R != 3 || S != 3) return ddlw_fail(who, "R and S must be 3");
  if (stride != 1) return ddlw_fail(who, "stride must be 1");
  if (pad != 1) return ddlw_fail(who, "pad must be 1");
  if (C % 64 != 0 || K % 64 != 0)
    return ddlw_fail(who, "C and K must be multiples of 64");
  if (N < 1 || H < 1 || W_ < 1 || W_ > 64)
    return ddlw_fail(who, "width must be 1..64");
  const long rows = (long)N * H;
  if ((long)N * (H + 1) * W_ >= (1ll << 31))
    return ddlw_fail(who, "N*(H+1)*W >= 2^31 unsupported");
  if (split < 1 || split > rows || split > 65535)
    return ddlw_fail(who, "split must be 1..min(N*H, 65535)");
  unsigned long long mg_h;
  unsigned sh_h;
  make_magic((unsigned)H, &mg_h, &sh_h);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((K / 64) * (C / 64), split);
  const int pw = W_ <= 8 ? 8 : W_ <= 16 ? 16 : W_ <= 32 ? 32 : 64;
  with_int<8, 16, 32, 64>(pw, [&](auto PWc) {
    hipLaunchKernelGGL((k_conv_wgrad3x3<decltype(PWc)::value>), grid,
                       dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)x,
                       (const bf16_t*)zpage, (float*)slab, N, H, W_, C, K,
                       (int)(rows / split), (int)(rows % split), mg_h, sh_h);
  });
  DDLW_CHECK_LAUNCH_OR_RETURN();
  long elems = (long)K * 9 * C;
  long g = cdiv(elems, 32);
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((int)g), dim3(256), 0, st,
                     (const float*)slab, (bf16_t*)dw, elems, split);
  DDLW_CHECK_LAUNCH();
}
