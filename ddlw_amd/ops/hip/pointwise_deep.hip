// Split-reduction pointwise (1x1, stride 1, pad 0) conv for the deep,
// grid-starved layers of the MobileNetV2 tail (576/960/1280-deep reductions
// over a few thousand rows). Same maths and contract as k_pw_conv in
// pointwise.hip:
//   y[m][k] = act((sum_c x[m][c] * w[k][c]) * scale[k] + bias[k] (+ res[m][k]))
// NHWC bf16 in/out, fp32 accumulation and epilogue, one rounding to bf16;
// C % 8 == 0, K % 8 == 0; scale/bias nullable together, res nullable.
//
// k_pw_conv gives a wave 32 rows and the WHOLE reduction: at C = 960 that is
// 30 dependent load -> MFMA steps per wave and, at 3136 rows, 25 blocks on 256
// CUs. Here the split of the work is the other way round:
//   - a block of 4 waves owns ONE tile of 16*MR rows x 32*NP output channels
//     (MR = 1, 2; NP as pw_pick_np picks it), so the grid is
//     cdiv(M, 16*MR) x ntiles blocks: 98 / 196 at 3136 rows instead of 25;
//   - the four waves split the reduction axis: wave v takes the 32-deep steps
//     s with s % 4 == v, so per round the block reads 256 contiguous bytes of
//     every x and w row and a wave's dependent chain is a quarter as long. A
//     wave with no step at all (C < 128) keeps zero accumulators and still
//     reaches every barrier;
//   - the loop is software-pipelined in registers: two fragment sets, the
//     loads of the wave's next step are issued before the MFMAs of the
//     current one;
//   - MFMA, fragment convention and tail staging are those of PW_TILE_MMA:
//     v_mfma_f32_16x16x32_bf16 with W as the A operand and x as the B operand,
//     one 16-byte load per lane and fragment, weight rows in the order
//     k = 8*(i>>2) + 4*f + (i&3) so a lane ends with 8 consecutive output
//     channels, and a row or vector past M / K / C loaded from a clamped
//     address and zeroed;
//   - the four partial tiles meet in LDS and are added in wave order
//     ((w0 + w1) + w2) + w3: no atomics, two calls are bit-equal. A "unit" is
//     one 16-row fragment x 32 channels (NP*MR of them); the reduce runs in
//     rounds of four units, one per wave, so the epilogue is spread over all
//     four waves: the wave that sums a unit loads scale/bias as float4 pairs
//     and res as one 16-byte load and writes y with one 16-byte store per
//     lane. One round holds 4 waves x 4 units x 2 KB = 32 KB of static LDS
//     (the whole 32 x 192 tile of four waves would be 96 KB), reused by the
//     next round behind a second barrier.
// Price: every block re-reads its whole W slab (2*C*32*NP bytes, 307 KB at
// 960 -> 160) from L2, 98 / 196 times instead of 25.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 pwd_bf16x8;
typedef __attribute__((ext_vector_type(4))) float pwd_f32x4;

#define PWD_WAVES 4
#define PWD_UR 4                   // units per reduce round: one per wave

// one 32-deep step of a wave as loaded: MR x fragments, NP pairs of W
// fragments, and whether the lane's channel vector lies inside C
template <int NP, int MR>
struct PwdFrag {
  union { uint4 u; pwd_bf16x8 v; } x[MR], w[NP][2];
  bool cok;
};

// clamped, in-bounds row pointers of a lane with their validity kept aside
template <int NP, int MR>
struct PwdRows {
  const bf16_t* xrow[MR];
  const bf16_t* wrow[NP][2];
  bool xok[MR];
  bool wok[NP][2];
};

// Issue the loads of the step at channel c0, all from in-bounds addresses.
// Nothing here reads a loaded value, so the wave does not wait for them.
template <int NP, int MR>
__device__ __forceinline__ void pwd_load(PwdFrag<NP, MR>& fr, const PwdRows<NP, MR>& r,
                                         int c0, int lg, int C) {
  const int c = c0 + lg * 8;
  fr.cok = c < C;                                // C % 8 == 0: whole vectors
  const int cc = fr.cok ? c : 0;
  #pragma unroll
  for (int mi = 0; mi < MR; ++mi)
    fr.x[mi].u = *reinterpret_cast<const uint4*>(r.xrow[mi] + cc);
  #pragma unroll
  for (int p = 0; p < NP; ++p)
    #pragma unroll
    for (int f = 0; f < 2; ++f)
      fr.w[p][f].u = *reinterpret_cast<const uint4*>(r.wrow[p][f] + cc);
}

// Zero what was loaded from a clamped address (the second half of the
// predicated staging, placed at the use so that it is the MFMAs of a step
// that wait for its loads), then the step's MFMAs.
template <int NP, int MR>
__device__ __forceinline__ void pwd_mma(pwd_f32x4 (&acc)[NP][2][MR],
                                        PwdFrag<NP, MR>& fr, const PwdRows<NP, MR>& r) {
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  #pragma unroll
  for (int mi = 0; mi < MR; ++mi)
    if (!(fr.cok && r.xok[mi])) fr.x[mi].u = zero;
  #pragma unroll
  for (int p = 0; p < NP; ++p)
    #pragma unroll
    for (int f = 0; f < 2; ++f) {
      if (!(fr.cok && r.wok[p][f])) fr.w[p][f].u = zero;
      #pragma unroll
      for (int mi = 0; mi < MR; ++mi)
        acc[p][f][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            fr.w[p][f].v, fr.x[mi].v, acc[p][f][mi], 0, 0, 0);
    }
}

// The wave's share of the tile product: acc[p][f][mi] over the 32-deep steps
// s = wave, wave + 4, ... of the block's 16*MR rows from m0 x 32*NP output
// channels from k0. Rows past M, weight rows past K, channel vectors past C
// and whole steps past the end contribute exactly zero.
template <int NP, int MR>
__device__ __forceinline__ void pwd_tile_mma(
    pwd_f32x4 (&acc)[NP][2][MR], const bf16_t* __restrict__ x,
    const bf16_t* __restrict__ w, long M, int C, int K, long m0, int k0,
    int wave, int l15, int lg) {
  PwdRows<NP, MR> r;
  #pragma unroll
  for (int mi = 0; mi < MR; ++mi) {
    const long m = m0 + mi * 16 + l15;
    r.xok[mi] = m < M;
    r.xrow[mi] = x + (r.xok[mi] ? m : M - 1) * C;
  }
  #pragma unroll
  for (int p = 0; p < NP; ++p)
    #pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int k = k0 + p * 32 + (l15 >> 2) * 8 + f * 4 + (l15 & 3);
      r.wok[p][f] = k < K;
      r.wrow[p][f] = w + (long)(r.wok[p][f] ? k : K - 1) * C;
    }
  #pragma unroll
  for (int p = 0; p < NP; ++p)
    #pragma unroll
    for (int f = 0; f < 2; ++f)
      #pragma unroll
      for (int mi = 0; mi < MR; ++mi) acc[p][f][mi] = pwd_f32x4{0.f, 0.f, 0.f, 0.f};

  // two fragment sets: the loads of step s + 4 are in flight under the MFMAs
  // of step s. A step past the last one is a read of channel 0 that is
  // zeroed, and its MFMAs are not branched around: they add exact zeros, and
  // behind a branch the compiler sinks the loads to the use, unpipelined.
  // PWD_PHASE() emits no instruction. Its empty asm is a compiler-only memory
  // fence: without it the optimizer merges the load before the loop with the
  // one at its end into one load at the top of the body, which puts every
  // load of an iteration in front of its MFMAs again. Its scheduling barrier
  // keeps the four phases of the body in this order in the emitted code.
#define PWD_PHASE()                  \
  asm volatile("" ::: "memory");     \
  __builtin_amdgcn_sched_barrier(0)
  const int steps = (C + 31) >> 5;
  PwdFrag<NP, MR> fa, fb;
  pwd_load(fa, r, wave * 32, lg, C);
  for (int s = wave; s < steps; s += 2 * PWD_WAVES) {
    pwd_load(fb, r, (s + PWD_WAVES) * 32, lg, C);
    PWD_PHASE();
    pwd_mma(acc, fa, r);
    PWD_PHASE();
    pwd_load(fa, r, (s + 2 * PWD_WAVES) * 32, lg, C);
    PWD_PHASE();
    pwd_mma(acc, fb, r);
    PWD_PHASE();
  }
#undef PWD_PHASE
}

// LDS of one reduce round: [wave][unit of the round][f][lane] float4, so each
// ds_write/read_b128 of a wave covers 64 consecutive 16-byte slots.
template <int NP, int MR>
struct PwdGeom {
  static constexpr int U = NP * MR;                          // units per tile
  static constexpr int UR = U < PWD_UR ? U : PWD_UR;         // per round
  static constexpr int ROUNDS = (U + PWD_UR - 1) / PWD_UR;
  static constexpr int SLOTS = PWD_WAVES * UR * 2 * 64;      // float4 slots
};

// Round `rd` of the cross-wave reduce: every wave publishes its partials of
// units 4*rd .. 4*rd+3, then wave v sums unit 4*rd + v of the four waves in
// wave order into v8 (lane (lg, l15): 8 consecutive channels of one row).
// Every thread of the block must call it. Returns the unit summed, or -1.
template <int NP, int MR>
__device__ __forceinline__ int pwd_reduce_round(
    const pwd_f32x4 (&acc)[NP][2][MR], float4* lds, int rd, int wave, int lane,
    float (&v8)[8]) {
  typedef PwdGeom<NP, MR> G;
  if (rd > 0) __syncthreads();                   // the previous round was read
  #pragma unroll
  for (int j = 0; j < G::UR; ++j) {
    const int u = rd * PWD_UR + j;
    if (u < G::U) {
      #pragma unroll
      for (int f = 0; f < 2; ++f) {
        const pwd_f32x4 a = acc[u / MR][f][u % MR];
        lds[((wave * G::UR + j) * 2 + f) * 64 + lane] = make_float4(a[0], a[1], a[2], a[3]);
      }
    }
  }
  __syncthreads();
  const int u = rd * PWD_UR + wave;
  if (wave >= G::UR || u >= G::U) return -1;
  #pragma unroll
  for (int f = 0; f < 2; ++f) {
    float4 t = lds[((0 * G::UR + wave) * 2 + f) * 64 + lane];
    #pragma unroll
    for (int wv = 1; wv < PWD_WAVES; ++wv) {
      const float4 o = lds[((wv * G::UR + wave) * 2 + f) * 64 + lane];
      t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
    }
    v8[f * 4 + 0] = t.x; v8[f * 4 + 1] = t.y; v8[f * 4 + 2] = t.z; v8[f * 4 + 3] = t.w;
  }
  return u;
}

template <int NP, int MR, bool HAS_RES>
__global__ __launch_bounds__(256) void k_pw_conv_deep(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ y, const bf16_t* __restrict__ res,
    const float* __restrict__ scale, const float* __restrict__ bias, int act,
    long M, int C, int K, int ntiles) {
  typedef PwdGeom<NP, MR> G;
  __shared__ __attribute__((aligned(16))) float4 lds[G::SLOTS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long mtile = blockIdx.x / ntiles;
  const int ntile = blockIdx.x - (int)(mtile * ntiles);
  const int l15 = lane & 15;
  const int lg = lane >> 4;                      // 0..3: channel group of 8
  const long m0 = mtile * (MR * 16);
  const int k0 = ntile * (NP * 32);

  pwd_f32x4 acc[NP][2][MR];
  pwd_tile_mma<NP, MR>(acc, x, w, M, C, K, m0, k0, wave, l15, lg);

  #pragma unroll
  for (int rd = 0; rd < G::ROUNDS; ++rd) {
    float v[8];
    const int u = pwd_reduce_round<NP, MR>(acc, lds, rd, wave, lane, v);
    if (u < 0) continue;
    const int kb = k0 + (u / MR) * 32 + lg * 8;
    const long m = m0 + (u % MR) * 16 + l15;
    if (kb >= K || m >= M) continue;
    const long oi = m * K + kb;
    if (scale) {
      float sc[8], bi[8];
      load8f(scale + kb, sc);
      load8f(bias + kb, bi);
      #pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = v[e] * sc[e] + bi[e];
    }
    if constexpr (HAS_RES) {
      bf16x8 rr;
      rr.v = *reinterpret_cast<const uint4*>(res + oi);
      #pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += b2f(rr.h[e]);
    }
    bf16x8 o;
    #pragma unroll
    for (int e = 0; e < 8; ++e) o.h[e] = f2b(apply_act(v[e], act));
    *reinterpret_cast<uint4*>(y + oi) = o.v;
  }
}

// k_pw_conv_deep_stats — the training forward on the same split: y = x * w^T
// with no epilogue maths (bit-equal to k_pw_conv_deep without scale, res and
// act: same accumulation chain, same reduce order) plus the BatchNorm
// statistics of the bf16-ROUNDED y as one partial row per row tile,
//   psum[mtile][k] = sum over the tile's 16*MR rows of y[m][k],  psq: of y^2.
// The wave that finishes a unit folds its 16 rows with row_sum16 and leaves
// 32 channel sums in LDS; after the last round the MR units of a channel are
// added in unit order, and block (mtile, ntile) alone writes row mtile of its
// own N tile's channels. Rows past M and channels past K are exact zeros and
// add nothing; only the stores are masked.
template <int NP, int MR>
__global__ __launch_bounds__(256) void k_pw_conv_deep_stats(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ y, float* __restrict__ psum, float* __restrict__ psq,
    long M, int C, int K, int ntiles) {
  typedef PwdGeom<NP, MR> G;
  __shared__ __attribute__((aligned(16))) float4 lds[G::SLOTS];
  __shared__ __attribute__((aligned(16))) float red[2][NP][MR][32];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long mtile = blockIdx.x / ntiles;
  const int ntile = blockIdx.x - (int)(mtile * ntiles);
  const int l15 = lane & 15;
  const int lg = lane >> 4;
  const long m0 = mtile * (MR * 16);
  const int k0 = ntile * (NP * 32);

  pwd_f32x4 acc[NP][2][MR];
  pwd_tile_mma<NP, MR>(acc, x, w, M, C, K, m0, k0, wave, l15, lg);

  #pragma unroll
  for (int rd = 0; rd < G::ROUNDS; ++rd) {
    float v[8];
    const int u = pwd_reduce_round<NP, MR>(acc, lds, rd, wave, lane, v);
    if (u < 0) continue;
    const int p = u / MR, mi = u % MR;
    const int kb = k0 + p * 32 + lg * 8;
    const long m = m0 + mi * 16 + l15;
    bf16x8 o;
    float s[8], q[8];
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
      o.h[e] = f2b(v[e]);
      const float r = b2f(o.h[e]);
      s[e] = row_sum16(r);
      q[e] = row_sum16(r * r);
    }
    if (m < M && kb < K) *reinterpret_cast<uint4*>(y + m * K + kb) = o.v;
    if (l15 == 0) {
      float* rs = &red[0][p][mi][lg * 8];
      float* rq = &red[1][p][mi][lg * 8];
      *reinterpret_cast<float4*>(rs) = make_float4(s[0], s[1], s[2], s[3]);
      *reinterpret_cast<float4*>(rs + 4) = make_float4(s[4], s[5], s[6], s[7]);
      *reinterpret_cast<float4*>(rq) = make_float4(q[0], q[1], q[2], q[3]);
      *reinterpret_cast<float4*>(rq + 4) = make_float4(q[4], q[5], q[6], q[7]);
    }
  }
  __syncthreads();
  const int t = threadIdx.x;                     // NP * 32 <= 192 < 256
  if (t < NP * 32 && k0 + t < K) {
    float ts = red[0][t >> 5][0][t & 31], tq = red[1][t >> 5][0][t & 31];
    #pragma unroll
    for (int mi = 1; mi < MR; ++mi) {
      ts += red[0][t >> 5][mi][t & 31];
      tq += red[1][t >> 5][mi][t & 31];
    }
    psum[mtile * K + k0 + t] = ts;
    psq[mtile * K + k0 + t] = tq;
  }
}

// pw_pick_np of pointwise.hip: the smallest listed NP that covers K in one
// tile, else whichever of 5 / 6 wastes fewer pairs over ceil(K/32).
static int pwd_pick_np(int K) {
  const int kp = (K + 31) / 32;
  if (kp <= 3) return kp;
  if (kp <= 5) return 5;
  if (kp == 6) return 6;
  const int w5 = (kp + 4) / 5 * 5, w6 = (kp + 5) / 6 * 6;
  return w5 < w6 ? 5 : 6;
}

// As ddlw_pw_conv_fwd (x [M][C], w [K][C], y/res [M][K] bf16; scale/bias fp32
// [K], both or neither) on the split-reduction kernel; mr = 1 or 2 16-row
// fragments per block tile.
DDLW_EXPORT int ddlw_pw_conv_deep_fwd(const void* x, const void* w, void* y,
                                      const void* res, const void* scale,
                                      const void* bias, int act, long M, int C,
                                      int K, int mr, void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("pw_conv_deep_fwd", why); };
  if (C <= 0 || C % 8 != 0 || K <= 0 || K % 8 != 0)
    return fail("C and K must be positive multiples of 8");
  if (M < 0 || M >= (1l << 31)) return fail("M must be below 2^31");
  if (act < 0 || act > 2) return fail("act must be 0, 1 or 2");
  if (mr != 1 && mr != 2) return fail("mr must be 1 or 2");
  if ((scale == nullptr) != (bias == nullptr))
    return fail("scale and bias come together");
  if ((((size_t)x | (size_t)w | (size_t)y | (size_t)res | (size_t)scale |
        (size_t)bias) & 15) != 0)
    return fail("pointers must be 16-byte aligned");
  if (M == 0) return 0;
  const int np = pwd_pick_np(K);
  const int ntiles = (K + np * 32 - 1) / (np * 32);
  const long blocks = cdiv(M, 16 * mr) * ntiles;
  if (blocks >= (1l << 31)) return fail("grid too large");
  with_int<1, 2, 3, 5, 6>(np, [&](auto NPc) {
    with_int<1, 2>(mr, [&](auto MRc) {
      with_bool(res != nullptr, [&](auto HR) {
        hipLaunchKernelGGL((k_pw_conv_deep<decltype(NPc)::value, decltype(MRc)::value,
                                           decltype(HR)::value>),
                           dim3((unsigned)blocks), dim3(256), 0,
                           (hipStream_t)stream, (const bf16_t*)x,
                           (const bf16_t*)w, (bf16_t*)y, (const bf16_t*)res,
                           (const float*)scale, (const float*)bias, act, M, C, K,
                           ntiles);
      });
    });
  });
  DDLW_CHECK_LAUNCH();
}

// Partial rows ddlw_pw_conv_deep_fwd_stats writes per channel: one per
// 16*mr-row tile. Launches nothing; -1 on a bad argument.
DDLW_EXPORT int ddlw_pw_conv_deep_nparts(long M, int mr, void* stream) {
  (void)stream;
  if (M < 0 || M >= (1l << 31) || (mr != 1 && mr != 2)) return -1;
  const long n = cdiv(M, 16 * mr);
  return n >= (1l << 31) ? -1 : (int)n;
}

// As ddlw_pw_conv_fwd_stats on the split-reduction kernel: y [M][K] bf16 and
// psum/psq fp32 [ddlw_pw_conv_deep_nparts(M, mr)][K].
DDLW_EXPORT int ddlw_pw_conv_deep_fwd_stats(const void* x, const void* w, void* y,
                                            void* psum, void* psq, long M, int C,
                                            int K, int mr, void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("pw_conv_deep_fwd_stats", why); };
  if (C <= 0 || C % 8 != 0 || K <= 0 || K % 8 != 0)
    return fail("C and K must be positive multiples of 8");
  if (M < 0 || M >= (1l << 31)) return fail("M must be below 2^31");
  if (mr != 1 && mr != 2) return fail("mr must be 1 or 2");
  if ((((size_t)x | (size_t)w | (size_t)y) & 15) != 0)
    return fail("x, w and y must be 16-byte aligned");
  if (psum == nullptr || psq == nullptr || (((size_t)psum | (size_t)psq) & 3) != 0)
    return fail("psum and psq must be fp32 buffers");
  if (M == 0) return 0;
  const int np = pwd_pick_np(K);
  const int ntiles = (K + np * 32 - 1) / (np * 32);
  const long blocks = cdiv(M, 16 * mr) * ntiles;
  if (blocks >= (1l << 31)) return fail("grid too large");
  with_int<1, 2, 3, 5, 6>(np, [&](auto NPc) {
    with_int<1, 2>(mr, [&](auto MRc) {
      hipLaunchKernelGGL((k_pw_conv_deep_stats<decltype(NPc)::value, decltype(MRc)::value>),
                         dim3((unsigned)blocks), dim3(256), 0,
                         (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)w,
                         (bf16_t*)y, (float*)psum, (float*)psq, M, C, K, ntiles);
    });
  });
  DDLW_CHECK_LAUNCH();
}
