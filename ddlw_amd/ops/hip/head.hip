// The two ends of the network around the conv stack: uint8 input normalize,
// and the classifier head — dropout, fused softmax + cross-entropy, row
// argmax and accuracy. Small memory-bound kernels; grids are capped at 2048
// workgroups of 256 threads with grid-stride loops.
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
__device__ __forceinline__ int ddlw_row_argmax(const float* row, int C) {
  const int lane = threadIdx.x & 63;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    float v = row[c];
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
