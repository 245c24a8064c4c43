// The two ends of the network around the conv stack: uint8 input normalize,
// and the classifier head — dropout, fused softmax + cross-entropy, row
// argmax and accuracy, and the one-pass loss + gradient + metrics step.
// Small memory-bound kernels; the element-wise ones cap their grids at 2048
// workgroups of 256 threads and stride, the row kernels put one wave on a
// row (k_ce_metrics: 1024 threads, one block or at most 256).
#include "common.h"

// ---------------------------------------------------------------------------
// Fused softmax + sparse cross-entropy, fwd+bwd in one pass (K9):
// logits fp32 [B, K] (the classifier head outputs fp32), labels i64.
// One wave per row: online max + sumexp via shuffle reduction, then
// dlogits = (softmax - onehot) * grad_scale, loss accumulated per row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_softmax_ce(
    const float* __restrict__ logits, const long* __restrict__ labels,
    float* __restrict__ dlogits, float* __restrict__ loss_sum,
    int B, int K, float grad_scale) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int b = wave; b < B; b += nwaves) {
    const float* row = logits + (long)b * K;
    float mx = -3.4e38f;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, row[k]);
    mx = warp_reduce_max(mx);
    mx = __shfl(mx, 0, 64);
    float se = 0.f;
    for (int k = lane; k < K; k += 64) se += __expf(row[k] - mx);
    se = warp_reduce_sum(se);
    se = __shfl(se, 0, 64);
    const float inv_se = 1.f / se;
    const long lab = labels[b];
    for (int k = lane; k < K; k += 64) {
      float p = __expf(row[k] - mx) * inv_se;
      dlogits[(long)b * K + k] = (p - (k == (int)lab ? 1.f : 0.f)) * grad_scale;
    }
    if (lane == 0) {
      float logp = row[lab] - mx - __logf(se);
      atomicAdd(loss_sum, -logp);
    }
  }
}

DDLW_EXPORT int ddlw_softmax_ce(const void* logits, const void* labels,
                                void* dlogits, void* loss_sum, int B, int K,
                                float grad_scale, void* stream) {
  int waves_needed = B;
  int blocks = min((waves_needed + 3) / 4, 1024);
  hipLaunchKernelGGL(k_softmax_ce, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                     (const float*)logits, (const long*)labels, (float*)dlogits,
                     (float*)loss_sum, B, K, grad_scale);
  DDLW_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// K7: Dropout fwd/bwd (head path, B x 1280 — reference P1/02:174, p tunable
// P2/01:197). Counter-based RNG (splitmix64 of (seed, index)): stateless,
// deterministic given the seed, no curand dependency. Bitmask layout = one
// byte per 8 elements (same convention as the BN ReLU mask).
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned ddlw_hash32(unsigned long long s) {
  s ^= s >> 33;
  s *= 0xff51afd7ed558ccdULL;
  s ^= s >> 33;
  s *= 0xc4ceb9fe1a85ec53ULL;
  s ^= s >> 33;
  return (unsigned)s;
}

__global__ __launch_bounds__(256) void k_dropout_fwd(
    const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
    unsigned char* __restrict__ mask, long n8, float p, float scale,
    unsigned long long seed) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += (long)gridDim.x * blockDim.x) {
    bf16x8 v, o;
    v.v = *reinterpret_cast<const uint4*>(x + i * 8);
    unsigned char mb = 0;
    #pragma unroll
    for (int k = 0; k < 8; ++k) {
      unsigned r = ddlw_hash32(seed + (unsigned long long)(i * 8 + k));
      bool keep = (float)(r >> 8) * (1.f / 16777216.f) >= p;
      if (keep) mb |= (1u << k);
      o.h[k] = keep ? f2b(b2f(v.h[k]) * scale) : (bf16_t)0;
    }
    *reinterpret_cast<uint4*>(y + i * 8) = o.v;
    mask[i] = mb;
  }
}

__global__ __launch_bounds__(256) void k_dropout_bwd(
    const bf16_t* __restrict__ dy, const unsigned char* __restrict__ mask,
    bf16_t* __restrict__ dx, long n8, float scale) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8;
       i += (long)gridDim.x * blockDim.x) {
    bf16x8 v, o;
    v.v = *reinterpret_cast<const uint4*>(dy + i * 8);
    unsigned char mb = mask[i];
    #pragma unroll
    for (int k = 0; k < 8; ++k)
      o.h[k] = ((mb >> k) & 1) ? f2b(b2f(v.h[k]) * scale) : (bf16_t)0;
    *reinterpret_cast<uint4*>(dx + i * 8) = o.v;
  }
}

DDLW_EXPORT int ddlw_dropout_fwd(const void* x, void* y, void* mask, long n,
                                 float p, unsigned long long seed,
                                 void* stream) {
  if (n % 8 != 0) return ddlw_fail("dropout", "n must be a multiple of 8");
  float scale = 1.f / (1.f - p);
  hipLaunchKernelGGL(k_dropout_fwd, dim3(grid_1d(n / 8)), dim3(256), 0,
                     (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y,
                     (unsigned char*)mask, n / 8, p, scale, seed);
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_dropout_bwd(const void* dy, const void* mask, void* dx,
                                 long n, float p, void* stream) {
  float scale = 1.f / (1.f - p);
  hipLaunchKernelGGL(k_dropout_bwd, dim3(grid_1d(n / 8)), dim3(256), 0,
                     (hipStream_t)stream, (const bf16_t*)dy,
                     (const unsigned char*)mask, (bf16_t*)dx, n / 8, scale);
  DDLW_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// K12: row argmax (inference: logits -> class index, P2/03:208-210) and
// K11: accuracy (argmax == label, per-block deterministic partial counts).
// One wave per row; first-max-index tie-break matches torch.argmax.
// ---------------------------------------------------------------------------
// T: float, or bf16_t (widened exactly, so the rule is the same)
template <class T>
__device__ __forceinline__ int ddlw_row_argmax(const T* row, int C) {
  const int lane = threadIdx.x & 63;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    float v;
    if constexpr (std::is_same_v<T, float>) v = row[c];
    else v = b2f(row[c]);
    if (v > best) { best = v; bi = c; }
  }
  #pragma unroll
  for (int off = 32; off; off >>= 1) {
    float ov = __shfl_down(best, off, 64);
    int oi = __shfl_down(bi, off, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  return bi;  // valid in lane 0
}

__global__ __launch_bounds__(256) void k_argmax_rows(
    const float* __restrict__ logits, long* __restrict__ out, long N, int C) {
  long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  int bi = ddlw_row_argmax(logits + row * C, C);
  if ((threadIdx.x & 63) == 0) out[row] = bi;
}

__global__ __launch_bounds__(256) void k_accuracy(
    const float* __restrict__ logits, const long* __restrict__ labels,
    int* __restrict__ partial, long N, int C) {
  long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  __shared__ int cnt[4];
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  __syncthreads();
  if (row < N) {
    int bi = ddlw_row_argmax(logits + row * C, C);
    if ((threadIdx.x & 63) == 0)
      cnt[threadIdx.x >> 6] = (bi == (int)labels[row]) ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    partial[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

DDLW_EXPORT int ddlw_argmax_rows(const void* logits, void* out, long N, int C,
                                 void* stream) {
  hipLaunchKernelGGL(k_argmax_rows, dim3((int)((N + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, (const float*)logits, (long*)out, N,
                     C);
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_accuracy(const void* logits, const void* labels,
                              void* partial, long N, int C, void* stream) {
  hipLaunchKernelGGL(k_accuracy, dim3((int)((N + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, (const float*)logits,
                     (const long*)labels, (int*)partial, N, C);
  DDLW_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// Loss, gradient and metrics of one step from the logits in one pass
// (k_ce_metrics): logits [B, K] bf16 or fp32 as the head produced them,
// labels i64. One wave per row, fp32 math, the max-subtracted softmax of
// k_softmax_ce and the argmax of k_accuracy. Writes
//   dlogits [B, K] (nullable; the logits' dtype) = (softmax - onehot) * scale
//   step_out fp32 [2] = {mean loss, correct / B}
//   accum fp64 [4] (nullable) += {mean loss, accuracy, 1, bad labels}
// A label outside [0, K) indexes nothing: zero loss, a zero dlogits row, not
// correct, counted. No atomics: a wave sums its rows in order, thread 0 the
// 16 waves of a block, and the blocks in index order, so two calls on the
// same input are bit-equal. One block when it can walk the rows
// (ddlw_ce_metrics_nblocks); otherwise per-block partials
// {loss fp32, correct i32, bad i32}[nblocks] and a one-thread finalize.
// ---------------------------------------------------------------------------
#define CE_WAVES 16  // waves (rows in flight) per 1024-thread block

__device__ __forceinline__ float ddlw_ldf(const float* p) { return *p; }
__device__ __forceinline__ float ddlw_ldf(const bf16_t* p) { return b2f(*p); }
__device__ __forceinline__ void ddlw_stf(float* p, float v) { *p = v; }
__device__ __forceinline__ void ddlw_stf(bf16_t* p, float v) { *p = f2b(v); }

// The build is -ffast-math, which turns the fp32 a / b into a * rcp(b), one
// ulp off (3 / 3 < 1), and accuracy is compared for equality with a host
// division. The fp64 quotient (an fp64 ulp or two off under fast-math)
// rounded to fp32 is the correctly rounded correct / B: for integers
// a <= b < 2^24, a / b is at least 2^-49 (relative) away from every midpoint
// between two fp32 values. B goes in as the integer: with both operands
// widened from fp32 the compiler narrows the division back to fp32.
__device__ __forceinline__ float ddlw_div_rn(double a, int b) {
  return (float)(a / (double)b);
}

__device__ __forceinline__ void ce_metrics_commit(
    float loss_sum, int correct, int bad, int B, float* __restrict__ step_out,
    double* __restrict__ accum) {
  const float loss = ddlw_div_rn((double)loss_sum, B);
  const float acc = ddlw_div_rn((double)correct, B);
  step_out[0] = loss;
  step_out[1] = acc;
  if (accum) {
    accum[0] += (double)loss;
    accum[1] += (double)acc;
    accum[2] += 1.0;
    accum[3] += (double)bad;
  }
}

template <class T, bool ONE>
__global__ __launch_bounds__(CE_WAVES * 64) void k_ce_metrics(
    const T* __restrict__ logits, const long* __restrict__ labels,
    T* __restrict__ dlogits, float* __restrict__ step_out,
    double* __restrict__ accum, float* __restrict__ part_loss,
    int* __restrict__ part_cnt, int B, int K, float grad_scale) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  float w_loss = 0.f;  // lane 0: this wave's rows, in row order
  int w_correct = 0, w_bad = 0;
  for (long b = (long)blockIdx.x * CE_WAVES + wid; b < B;
       b += (long)gridDim.x * CE_WAVES) {
    const T* row = logits + b * K;
    const long lab = labels[b];
    const bool ok = lab >= 0 && lab < K;  // wave-uniform
    const int bi = ddlw_row_argmax(row, K);
    float mx = -3.4e38f;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, ddlw_ldf(row + k));
    mx = warp_reduce_max(mx);
    mx = __shfl(mx, 0, 64);
    float se = 0.f;
    for (int k = lane; k < K; k += 64) se += __expf(ddlw_ldf(row + k) - mx);
    se = warp_reduce_sum(se);
    se = __shfl(se, 0, 64);
    if (dlogits) {
      T* drow = dlogits + b * K;
      const float inv_se = 1.f / se;
      for (int k = lane; k < K; k += 64) {
        float p = __expf(ddlw_ldf(row + k) - mx) * inv_se;
        float g = (p - (k == (int)lab ? 1.f : 0.f)) * grad_scale;
        ddlw_stf(drow + k, ok ? g : 0.f);
      }
    }
    if (lane == 0) {
      if (ok) {
        w_loss += -(ddlw_ldf(row + lab) - mx - __logf(se));
        w_correct += (bi == (int)lab) ? 1 : 0;
      } else {
        w_bad += 1;
      }
    }
  }
  __shared__ float s_loss[CE_WAVES];
  __shared__ int s_correct[CE_WAVES], s_bad[CE_WAVES];
  if (lane == 0) {
    s_loss[wid] = w_loss;
    s_correct[wid] = w_correct;
    s_bad[wid] = w_bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float loss = 0.f;
    int correct = 0, bad = 0;
    for (int w = 0; w < CE_WAVES; ++w) {
      loss += s_loss[w];
      correct += s_correct[w];
      bad += s_bad[w];
    }
    if constexpr (ONE) {
      ce_metrics_commit(loss, correct, bad, B, step_out, accum);
    } else {
      part_loss[blockIdx.x] = loss;
      part_cnt[blockIdx.x] = correct;
      part_cnt[gridDim.x + blockIdx.x] = bad;
    }
  }
}

__global__ __launch_bounds__(64) void k_ce_metrics_finalize(
    const float* __restrict__ part_loss, const int* __restrict__ part_cnt,
    int nblocks, int B, float* __restrict__ step_out,
    double* __restrict__ accum) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float loss = 0.f;
  int correct = 0, bad = 0;
  for (int i = 0; i < nblocks; ++i) {
    loss += part_loss[i];
    correct += part_cnt[i];
    bad += part_cnt[nblocks + i];
  }
  ce_metrics_commit(loss, correct, bad, B, step_out, accum);
}

// Blocks the rows kernel runs for [B, K] logits; 1 = the single launch.
// One block walks up to 256K logits (batch 256 x 1000 classes: 16 rows per
// wave); above that, one row per wave up to 256 blocks, which keeps the
// finalize's serial sum short.
static inline int ce_metrics_nblocks(long B, long K) {
  if (B * K <= 256L * 1024) return 1;
  long nb = cdiv(B, CE_WAVES);
  return (int)(nb < 256 ? (nb > 2 ? nb : 2) : 256);
}

// Launches nothing; `stream` is there because every export outside the ABI
// test's pinned query list ends in one.
DDLW_EXPORT int ddlw_ce_metrics_nblocks(int B, int K, void* stream) {
  (void)stream;
  if (B <= 0 || K <= 0) return 0;
  return ce_metrics_nblocks(B, K);
}

// partials: 3 * nblocks 4-byte words of workspace, needed when nblocks > 1
DDLW_EXPORT int ddlw_ce_metrics(const void* logits, const void* labels,
                                void* dlogits, void* step_out, void* accum,
                                void* partials, int B, int K, float grad_scale,
                                int is_bf16, void* stream) {
  if (B <= 0 || K <= 0) return ddlw_fail("ce_metrics", "B and K must be positive");
  if (!logits || !labels) return ddlw_fail("ce_metrics", "logits and labels must not be null");
  if (!step_out) return ddlw_fail("ce_metrics", "step_out must not be null");
  const int nb = ce_metrics_nblocks(B, K);
  if (nb > 1 && !partials)
    return ddlw_fail("ce_metrics", "this shape needs the partials workspace");
  float* part_loss = (float*)partials;
  int* part_cnt = partials ? (int*)partials + nb : nullptr;
  with_bool(is_bf16 != 0, [&](auto bf) {
    using T = std::conditional_t<decltype(bf)::value, bf16_t, float>;
    with_bool(nb == 1, [&](auto one) {
      hipLaunchKernelGGL((k_ce_metrics<T, decltype(one)::value>), dim3(nb),
                         dim3(CE_WAVES * 64), 0, (hipStream_t)stream,
                         (const T*)logits, (const long*)labels, (T*)dlogits,
                         (float*)step_out, (double*)accum, part_loss, part_cnt,
                         B, K, grad_scale);
    });
  });
  if (nb > 1)
    hipLaunchKernelGGL(k_ce_metrics_finalize, dim3(1), dim3(64), 0,
                       (hipStream_t)stream, (const float*)part_loss,
                       (const int*)part_cnt, nb, B, (float*)step_out,
                       (double*)accum);
  DDLW_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// Input normalize: uint8 NHWC -> bf16 NHWC, x/127.5 - 1 (the MobileNetV2
// preprocess_input transform, reference P1/02:126), fused with the H2D'd
// uint8 batch so the fp32 intermediate never exists.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_normalize_u8(
    const unsigned char* __restrict__ x, bf16_t* __restrict__ y, long n16 /* n/16 */) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16;
       i += (long)gridDim.x * blockDim.x) {
    uint4 v = *reinterpret_cast<const uint4*>(x + i * 16);
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&v);
    bf16x8 o0, o1;
    #pragma unroll
    for (int k = 0; k < 8; ++k) o0.h[k] = f2b((float)b[k] * (1.f / 127.5f) - 1.f);
    #pragma unroll
    for (int k = 0; k < 8; ++k) o1.h[k] = f2b((float)b[8 + k] * (1.f / 127.5f) - 1.f);
    *reinterpret_cast<uint4*>(y + i * 16) = o0.v;
    *reinterpret_cast<uint4*>(y + i * 16 + 8) = o1.v;
  }
}

DDLW_EXPORT int ddlw_normalize_u8(const void* x, void* y, long n, void* stream) {
  hipLaunchKernelGGL(k_normalize_u8, dim3(grid_1d(n / 16)), dim3(256), 0,
                     (hipStream_t)stream, (const unsigned char*)x, (bf16_t*)y,
                     n / 16);
  DDLW_CHECK_LAUNCH();
}
