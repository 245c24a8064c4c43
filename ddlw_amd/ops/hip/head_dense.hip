// The classifier head between the pooled features and the loss: dropout +
// dense (C -> K classes, K <= 64) forward and backward, one launch each.
//   x  bf16 [N][C] pooled features, w bf16 [K][C], b bf16 [K] or null
//   xd[n,c] = keep(n*C+c) ? bf16(x[n,c]*scale) : 0
// with keep and scale exactly k_dropout_fwd's (head.hip): ddlw_hash32(seed +
// flat index), (float)(r >> 8) * 2^-24 >= p, scale = 1/(1-p); xd is bit-equal
// to what ddlw_dropout_fwd writes. Neither xd nor a mask is stored: forward
// and backward regenerate them from (x, seed, p) in registers.
//   logits[n,k] = bf16(sum_c xd[n,c]*w[k,c] + b[k])           (forward)
//   dW[k,c]     = bf16(sum_n dl[n,k]*xd[n,c])                 (backward)
//   db[k]       = bf16(sum_n dl[n,k])                         (nullable)
//   dx[n,c]     = keep ? bf16(scale * sum_k dl[n,k]*w[k,c]) : 0   (nullable)
// dl is dlogits in bf16, or in fp32 rounded to bf16 once as it is loaded.
// fp32 accumulation, one rounding per output, no atomics, fixed summation
// order: two calls are bit-equal. C % 8 == 0, C >= 8, 1 <= K <= 64, N >= 1.
//
// Both use v_mfma_f32_16x16x32_bf16 with the classes on the A operand (K
// padded to KF = ceil(K/16) fragments of 16 rows): an output lane (l15, lg)
// holds classes 16*kf + 4*lg + 0..3 of column l15.
//
// Forward (k_head_dense_fwd<KF, DROP>): grid-starved, batch 64 is four 16-row
// fragments and the reduction is 1280 deep, so the split of pointwise_deep.hip
// is turned inward. A workgroup of 8 waves owns 16 batch rows (the B operand);
// wave v takes the 32-deep steps s with s % 8 == v (per round the workgroup
// reads 512 contiguous bytes of each row), applies the dropout to the 8
// elements of its B vector in registers, and keeps KF accumulators. The eight
// partial tiles meet in LDS and wave kf adds fragment kf in wave order
// ((w0 + w1) + ... + w7), adds the bias and stores. DROP = false is the plain
// dense layer (eval, predict, p = 0): xd = x, no hashing.
//
// Backward (k_head_dense_bwd<KF, F32, DX>): the dW reduction runs over the
// batch index, the slow index of both x and dl, so both MFMA operands need it
// transposed into lanes. A workgroup of 4 waves owns 64 columns of C (16 per
// wave, one B fragment) and loops over the batch in steps of 32 rows; dW needs
// no fold across workgroups. Per step the 256 threads load the 32 x 64 slab of
// x as one 16-byte vector each (thread t: row t/8, vector t%8), apply the
// dropout, and write the 8 values TRANSPOSED into LDS (xsT[c][n], 2-byte
// writes, rows of 32 + 8 pad = 80 bytes); the 32 x K slab of dl goes the same
// way (dlT[k][n]). Each MFMA operand is then one ds_read_b128 of 8
// consecutive batch rows. db: in workgroup 0, thread k < K adds row k of dlT
// in batch order. dx (DX) is not a second phase: the thread that staged
// (row, vector) of x still holds its keep bits, so in the same step it forms
// sum_k dlT[k][row] * w[k][8 columns] with plain FMAs from the workgroup's
// K x 64 slab of w in LDS (natural layout, one ds_read_b128 per class). At
// K <= 64 and typically K = 5 an MFMA over K padded to 32 would multiply
// mostly zeros and need a third transposed operand.
// Rows past N, vectors past C and classes past K are loaded from clamped
// in-bounds addresses and zeroed; only stores are masked.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 hd_bf16x8;
typedef __attribute__((ext_vector_type(4))) float hd_f32x4;
union hd_frag { uint4 u; hd_bf16x8 v; };

#define HD_MAX_K 64
#define HD_FWD_WAVES 8
#define HD_BWD_CT 64                 // dW columns per workgroup: 16 per wave
#define HD_NS 32                     // batch rows per step: one MFMA depth
#define HD_LD (HD_NS + 8)            // LDS row stride, bf16: 80 B, 16-B aligned

// x[flat .. flat+8) -> xd in place; returns the keep bits. The expressions
// are k_dropout_fwd's, so the values are too.
__device__ __forceinline__ unsigned hd_dropout8(bf16x8& v, u64 seed, long flat,
                                                float p, float scale) {
  unsigned bits = 0;
  #pragma unroll
  for (int k = 0; k < 8; ++k) {
    unsigned r = ddlw_hash32(seed + (unsigned long long)(flat + k));
    bool keep = (float)(r >> 8) * (1.f / 16777216.f) >= p;
    if (keep) bits |= (1u << k);
    v.h[k] = keep ? f2b(b2f(v.h[k]) * scale) : (bf16_t)0;
  }
  return bits;
}

template <int KF, bool DROP>
__global__ __launch_bounds__(HD_FWD_WAVES * 64) void k_head_dense_fwd(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    const bf16_t* __restrict__ b, bf16_t* __restrict__ y, long N, int C, int K,
    float p, float scale, u64 seed) {
  __shared__ __attribute__((aligned(16))) float4 lds[HD_FWD_WAVES * KF * 64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l15 = lane & 15;
  const int lg = lane >> 4;                      // 0..3: channel group of 8
  const long m = (long)blockIdx.x * 16 + l15;
  const bool xok = m < N;
  const long xbase = (xok ? m : N - 1) * C;      // flat index of the row
  const bf16_t* wrow[KF];
  bool wok[KF];
  #pragma unroll
  for (int kf = 0; kf < KF; ++kf) {
    const int k = kf * 16 + l15;
    wok[kf] = k < K;
    wrow[kf] = w + (long)(wok[kf] ? k : K - 1) * C;
  }
  hd_f32x4 acc[KF];
  #pragma unroll
  for (int kf = 0; kf < KF; ++kf) acc[kf] = hd_f32x4{0.f, 0.f, 0.f, 0.f};

  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  const int steps = (C + 31) >> 5;
  for (int s = wave; s < steps; s += HD_FWD_WAVES) {
    const int c = s * 32 + lg * 8;
    const bool cok = c < C;                      // C % 8 == 0: whole vectors
    const int cc = cok ? c : 0;
    bf16x8 xv;
    xv.v = *reinterpret_cast<const uint4*>(x + xbase + cc);
    hd_frag wf[KF];
    #pragma unroll
    for (int kf = 0; kf < KF; ++kf)
      wf[kf].u = *reinterpret_cast<const uint4*>(wrow[kf] + cc);
    if constexpr (DROP) hd_dropout8(xv, seed, xbase + cc, p, scale);
    hd_frag xf;
    xf.u = (cok && xok) ? xv.v : zero;
    #pragma unroll
    for (int kf = 0; kf < KF; ++kf) {
      if (!(cok && wok[kf])) wf[kf].u = zero;
      acc[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[kf].v, xf.v, acc[kf], 0, 0, 0);
    }
  }

  #pragma unroll
  for (int kf = 0; kf < KF; ++kf)
    lds[(wave * KF + kf) * 64 + lane] =
        make_float4(acc[kf][0], acc[kf][1], acc[kf][2], acc[kf][3]);
  __syncthreads();
  if (wave >= KF) return;                        // wave kf finishes fragment kf
  float4 t = lds[(0 * KF + wave) * 64 + lane];
  #pragma unroll
  for (int wv = 1; wv < HD_FWD_WAVES; ++wv) {
    const float4 o = lds[(wv * KF + wave) * 64 + lane];
    t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
  }
  if (!xok) return;
  const float v[4] = {t.x, t.y, t.z, t.w};
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = wave * 16 + lg * 4 + r;
    if (k < K) y[m * K + k] = f2b(v[r] + (b ? b2f(b[k]) : 0.f));
  }
}

template <int KF, bool F32, bool DX>
__global__ __launch_bounds__(256) void k_head_dense_bwd(
    const void* __restrict__ dl_, const bf16_t* __restrict__ x,
    const bf16_t* __restrict__ w, bf16_t* __restrict__ dW,
    bf16_t* __restrict__ db, bf16_t* __restrict__ dx, long N, int C, int K,
    float p, float scale, u64 seed) {
  constexpr int KP = KF * 16;
  __shared__ __attribute__((aligned(16))) bf16_t xsT[HD_BWD_CT * HD_LD];
  __shared__ __attribute__((aligned(16))) bf16_t dlT[KP * HD_LD];
  __shared__ __attribute__((aligned(16))) bf16_t ws[DX ? KP * HD_BWD_CT : 8];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int l15 = lane & 15;
  const int lg = lane >> 4;
  const int c0 = blockIdx.x * HD_BWD_CT;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  // staging role: row nl of the step, 8 columns from c
  const int nl = t >> 3;
  const int cv = t & 7;
  const int c = c0 + cv * 8;
  const bool cok = c < C;
  const int cc = cok ? c : 0;

  if constexpr (DX) {
    for (int e = t; e < KP * (HD_BWD_CT / 8); e += 256) {
      const int k = e >> 3, v = e & 7;
      const int cw = c0 + v * 8;
      const bool ok = k < K && cw < C;
      uint4 wv = *reinterpret_cast<const uint4*>(w + (ok ? (long)k * C + cw : 0));
      if (!ok) wv = zero;
      *reinterpret_cast<uint4*>(&ws[k * HD_BWD_CT + v * 8]) = wv;
    }
  }

  hd_f32x4 acc[KF];
  #pragma unroll
  for (int kf = 0; kf < KF; ++kf) acc[kf] = hd_f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;
  const bool does_db = db != nullptr && blockIdx.x == 0 && t < K;

  for (long n0 = 0; n0 < N; n0 += HD_NS) {
    const long n = n0 + nl;
    const bool nok = n < N;
    const long flat = (nok ? n : N - 1) * C + cc;
    bf16x8 xv;
    xv.v = *reinterpret_cast<const uint4*>(x + flat);
    // p == 0 (uniform): xd = x, every element kept
    const unsigned keep = p > 0.f ? hd_dropout8(xv, seed, flat, p, scale) : 0xffu;
    if (!(nok && cok)) xv.v = zero;
    __syncthreads();                             // the previous step was read
    #pragma unroll
    for (int j = 0; j < 8; ++j) xsT[(cv * 8 + j) * HD_LD + nl] = xv.h[j];
    for (int e = t; e < HD_NS * KP; e += 256) {
      const int r = e / KP, k = e % KP;
      const bool ok = n0 + r < N && k < K;
      const long di = ok ? (n0 + r) * K + k : 0;
      bf16_t v;
      if constexpr (F32) v = f2b(reinterpret_cast<const float*>(dl_)[di]);
      else v = reinterpret_cast<const bf16_t*>(dl_)[di];
      dlT[k * HD_LD + r] = ok ? v : (bf16_t)0;
    }
    __syncthreads();

    hd_frag bx;
    bx.u = *reinterpret_cast<const uint4*>(&xsT[(wave * 16 + l15) * HD_LD + lg * 8]);
    #pragma unroll
    for (int kf = 0; kf < KF; ++kf) {
      hd_frag a;
      a.u = *reinterpret_cast<const uint4*>(&dlT[(kf * 16 + l15) * HD_LD + lg * 8]);
      acc[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, bx.v, acc[kf], 0, 0, 0);
    }
    if (does_db) {
      #pragma unroll
      for (int r = 0; r < HD_NS; ++r) dbacc += b2f(dlT[t * HD_LD + r]);
    }
    if constexpr (DX) {
      float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < K; ++k) {
        const float d = b2f(dlT[k * HD_LD + nl]);
        bf16x8 wv;
        wv.v = *reinterpret_cast<const uint4*>(&ws[k * HD_BWD_CT + cv * 8]);
        #pragma unroll
        for (int j = 0; j < 8; ++j) a8[j] += d * b2f(wv.h[j]);
      }
      bf16x8 o;
      #pragma unroll
      for (int j = 0; j < 8; ++j)
        o.h[j] = ((keep >> j) & 1) ? f2b(a8[j] * scale) : (bf16_t)0;
      if (nok && cok) *reinterpret_cast<uint4*>(dx + flat) = o.v;
    }
  }

  const int co = c0 + wave * 16 + l15;
  #pragma unroll
  for (int kf = 0; kf < KF; ++kf)
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = kf * 16 + lg * 4 + r;
      if (k < K && co < C) dW[(long)k * C + co] = f2b(acc[kf][r]);
    }
  if (does_db) db[t] = f2b(dbacc);
}

static int hd_check(const char* who, long N, int C, int K, float p) {
  if (C < 8 || C % 8 != 0) return ddlw_fail(who, "C must be a positive multiple of 8");
  if (K < 1 || K > HD_MAX_K) return ddlw_fail(who, "K must be in [1, 64]");
  if (N < 1 || N >= (1l << 31)) return ddlw_fail(who, "N must be in [1, 2^31)");
  if (!(p >= 0.f && p < 1.f)) return ddlw_fail(who, "p must be in [0, 1)");
  return 0;
}

// logits [N][K] bf16 from x [N][C], w [K][C], b [K] (nullable), all bf16.
// p > 0: the training variant, xd = dropout(x, p, seed); p == 0: plain dense.
DDLW_EXPORT int ddlw_head_dense_fwd(const void* x, const void* w, const void* b,
                                    void* y, long N, int C, int K, float p,
                                    unsigned long long seed, void* stream) {
  const char* who = "head_dense_fwd";
  if (int st = hd_check(who, N, C, K, p)) return st;
  if (!x || !w || !y) return ddlw_fail(who, "x, w and y must not be null");
  if ((((size_t)x | (size_t)w) & 15) != 0)
    return ddlw_fail(who, "x and w must be 16-byte aligned");
  const float scale = 1.f / (1.f - p);
  with_int<1, 2, 3, 4>((K + 15) / 16, [&](auto KFc) {
    with_bool(p > 0.f, [&](auto DR) {
      hipLaunchKernelGGL((k_head_dense_fwd<decltype(KFc)::value, decltype(DR)::value>),
                         dim3((unsigned)cdiv(N, 16)), dim3(HD_FWD_WAVES * 64), 0,
                         (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)w,
                         (const bf16_t*)b, (bf16_t*)y, N, C, K, p, scale, seed);
    });
  });
  DDLW_CHECK_LAUNCH();
}

// dW [K][C], db [K] (nullable), dx [N][C] (nullable) bf16 from dl [N][K]
// (fp32 if dl_f32, else bf16), x, w and the forward's (p, seed).
DDLW_EXPORT int ddlw_head_dense_bwd(const void* dl, const void* x, const void* w,
                                    void* dW, void* db, void* dx, long N, int C,
                                    int K, float p, unsigned long long seed,
                                    int dl_f32, void* stream) {
  const char* who = "head_dense_bwd";
  if (int st = hd_check(who, N, C, K, p)) return st;
  if (!dl || !x || !w || !dW) return ddlw_fail(who, "dl, x, w and dW must not be null");
  if ((((size_t)x | (size_t)w | (size_t)dx) & 15) != 0)
    return ddlw_fail(who, "x, w and dx must be 16-byte aligned");
  if (((size_t)dl & (dl_f32 ? 3 : 1)) != 0)
    return ddlw_fail(who, "dl must be aligned to its element");
  const float scale = 1.f / (1.f - p);
  with_int<1, 2, 3, 4>((K + 15) / 16, [&](auto KFc) {
    with_bool(dl_f32 != 0, [&](auto F) {
      with_bool(dx != nullptr, [&](auto D) {
        hipLaunchKernelGGL((k_head_dense_bwd<decltype(KFc)::value, decltype(F)::value,
                                             decltype(D)::value>),
                           dim3((unsigned)cdiv(C, HD_BWD_CT)), dim3(256), 0,
                           (hipStream_t)stream, dl, (const bf16_t*)x,
                           (const bf16_t*)w, (bf16_t*)dW, (bf16_t*)db, (bf16_t*)dx,
                           N, C, K, p, scale, seed);
      });
    });
  });
  DDLW_CHECK_LAUNCH();
}
