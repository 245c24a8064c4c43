// Pooling kernels of the ResNet / MobileNetV2 training step, NHWC bf16:
// max-pool 3x3 stride 2 (fwd + argmax-gather bwd) and global average pooling
// (fwd + bwd). Memory-bound: 16-byte bf16x8 accesses, fp32 accumulation.
#include "common.h"

// ---------------------------------------------------------------------------
// MaxPool 3x3 stride 2 pad 1, NHWC (the ResNet stem pool; K "maxpool" row).
// fwd records the argmax window slot (0..8) for an atomics-free backward.
// One thread per 8-channel vector of one output pixel.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_maxpool3x3s2_fwd(
    const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
    unsigned char* __restrict__ argmax,
    int N, int H, int W, int C, int Ho, int Wo) {
  const int vecC = C >> 3;
  // 32-bit index math: launcher guards total < 2^31 (the 64-bit div/mod
  // chain per grid-stride iteration was a measurable cost on this kernel)
  const unsigned total = (unsigned)((long)N * Ho * Wo * vecC);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += gridDim.x * blockDim.x) {
    unsigned vc = i % (unsigned)vecC;
    unsigned t = i / (unsigned)vecC;
    int wo = (int)(t % (unsigned)Wo); t /= (unsigned)Wo;
    int ho = (int)(t % (unsigned)Ho); t /= (unsigned)Ho;
    int n = (int)t;
    float best[8];
    int bidx[8];
    #pragma unroll
    for (int k = 0; k < 8; ++k) { best[k] = -3.4e38f; bidx[k] = 0; }
    #pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      int h = ho * 2 - 1 + kh;
      if (h < 0 || h >= H) continue;
      #pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        int w = wo * 2 - 1 + kw;
        if (w < 0 || w >= W) continue;
        bf16x8 v;
        v.v = *reinterpret_cast<const uint4*>(
            x + (((long)n * H + h) * W + w) * C + (long)vc * 8);
        #pragma unroll
        for (int k = 0; k < 8; ++k) {
          float f = b2f(v.h[k]);
          if (f > best[k]) { best[k] = f; bidx[k] = kh * 3 + kw; }
        }
      }
    }
    bf16x8 o;
    #pragma unroll
    for (int k = 0; k < 8; ++k) o.h[k] = f2b(best[k]);
    *reinterpret_cast<uint4*>(y + (long)i * 8) = o.v;
    // one 8-byte store instead of 8 byte-stores
    uint2 am;
    am.x = (unsigned)bidx[0] | ((unsigned)bidx[1] << 8) |
           ((unsigned)bidx[2] << 16) | ((unsigned)bidx[3] << 24);
    am.y = (unsigned)bidx[4] | ((unsigned)bidx[5] << 8) |
           ((unsigned)bidx[6] << 16) | ((unsigned)bidx[7] << 24);
    *reinterpret_cast<uint2*>(argmax + (long)i * 8) = am;
  }
}

// backward: gather — for each input element, sum dy over the <=4 output
// windows that could have selected it, checking the recorded argmax.
// grid: y = (n*H + h) input row, x covers w * vecC — one vector per
// thread, addresses by shift/mask (vecC is a power of two for every
// ResNet/MobileNet C) instead of the per-iteration div/mod chains of the
// old grid-stride form (which dominated this latency-bound kernel)
__global__ __launch_bounds__(256) void k_maxpool3x3s2_bwd(
    const bf16_t* __restrict__ dy, const unsigned char* __restrict__ argmax,
    bf16_t* __restrict__ dx,
    int N, int H, int W, int C, int Ho, int Wo, int lv /* log2(C/8) */) {
  const int vecC = C >> 3;
  {
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (unsigned)(W << lv)) return;
    const int w = (int)(idx >> lv);
    const unsigned vc = idx & ((1u << lv) - 1);
    const int h = blockIdx.y % (unsigned)H;
    const int n = blockIdx.y / (unsigned)H;
    const unsigned long long i =
        (((unsigned long long)blockIdx.y * W + w) << lv) + vc;
    float acc[8] = {0};
    // output windows covering (h, w): ho*2-1 <= h <= ho*2+1
    int ho_lo = (h - 1 + 1) / 2, ho_hi = (h + 1) / 2;  // ceil((h-1)/2), floor((h+1)/2)
    if (h == 0) ho_lo = 0;
    int wo_lo = (w - 1 + 1) / 2, wo_hi = (w + 1) / 2;
    if (w == 0) wo_lo = 0;
    for (int ho = ho_lo; ho <= ho_hi && ho < Ho; ++ho) {
      int kh = h - (ho * 2 - 1);
      if (kh < 0 || kh > 2) continue;
      for (int wo = wo_lo; wo <= wo_hi && wo < Wo; ++wo) {
        int kw = w - (wo * 2 - 1);
        if (kw < 0 || kw > 2) continue;
        long obase = (((long)n * Ho + ho) * Wo + wo) * C + (long)vc * 8;
        bf16x8 g;
        g.v = *reinterpret_cast<const uint4*>(dy + obase);
        // one 8-byte argmax load instead of 8 byte-loads
        uint2 am = *reinterpret_cast<const uint2*>(argmax + obase);
        unsigned slot = (unsigned)(kh * 3 + kw);
        #pragma unroll
        for (int k = 0; k < 8; ++k) {
          unsigned b = ((k < 4 ? am.x : am.y) >> ((k & 3) * 8)) & 0xffu;
          if (b == slot) acc[k] += b2f(g.h[k]);
        }
      }
    }
    bf16x8 o;
    #pragma unroll
    for (int k = 0; k < 8; ++k) o.h[k] = f2b(acc[k]);
    *reinterpret_cast<uint4*>(dx + (long)i * 8) = o.v;
  }
}

// ---------------------------------------------------------------------------
// Global average pooling NHWC: y[n,c] = mean_hw x[n,h,w,c]  (K6).
// One block per image n; threads own channel vectors; loop over H*W rows.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gap_fwd(
    const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
    int HW, int C) {
  const int vecC = C >> 3;
  const int n = blockIdx.x;
  const float inv = 1.f / (float)HW;
  for (int vc = threadIdx.x; vc < vecC; vc += blockDim.x) {
    float acc[8] = {0};
    const bf16_t* base = x + (long)n * HW * C + (long)vc * 8;
    for (int r = 0; r < HW; ++r) {
      bf16x8 v;
      v.v = *reinterpret_cast<const uint4*>(base + (long)r * C);
      #pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += b2f(v.h[k]);
    }
    bf16x8 o;
    #pragma unroll
    for (int k = 0; k < 8; ++k) o.h[k] = f2b(acc[k] * inv);
    *reinterpret_cast<uint4*>(y + (long)n * C + (long)vc * 8) = o.v;
  }
}

__global__ __launch_bounds__(256) void k_gap_bwd(
    const bf16_t* __restrict__ dy, bf16_t* __restrict__ dx,
    int HW, int C, long total /* N*HW*vecC */) {
  const int vecC = C >> 3;
  const float inv = 1.f / (float)HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    int vc = (int)(i % vecC);
    long n = i / ((long)vecC * HW);
    bf16x8 g, o;
    g.v = *reinterpret_cast<const uint4*>(dy + n * C + (long)vc * 8);
    #pragma unroll
    for (int k = 0; k < 8; ++k) o.h[k] = f2b(b2f(g.h[k]) * inv);
    *reinterpret_cast<uint4*>(dx + i * 8) = o.v;
  }
}

DDLW_EXPORT int ddlw_maxpool3x3s2_fwd(const void* x, void* y, void* argmax,
                                      int N, int H, int W, int C, int Ho, int Wo,
                                      void* stream) {
  long total = (long)N * Ho * Wo * (C >> 3);
  if ((long)N * H * W * (C >> 3) >= (1ll << 31))
    return ddlw_fail("maxpool3x3s2", "tensor too large for 32-bit indexing");
  hipLaunchKernelGGL(k_maxpool3x3s2_fwd, dim3(grid_1d(total)), dim3(256), 0,
                     (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y,
                     (unsigned char*)argmax, N, H, W, C, Ho, Wo);
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_maxpool3x3s2_bwd(const void* dy, const void* argmax, void* dx,
                                      int N, int H, int W, int C, int Ho, int Wo,
                                      void* stream) {
  int vecC = C >> 3;
  if (vecC <= 0 || (vecC & (vecC - 1)) != 0)
    return ddlw_fail("maxpool3x3s2_bwd", "C/8 must be a power of two");
  if ((long)N * H >= 65536 || (long)H * W * vecC >= (1ll << 31))
    return ddlw_fail("maxpool3x3s2", "tensor too large for the 2D grid");
  int lv = 0;
  while ((1 << lv) < vecC) ++lv;
  dim3 grid(((W << lv) + 255) / 256, N * H);
  hipLaunchKernelGGL(k_maxpool3x3s2_bwd, grid, dim3(256), 0,
                     (hipStream_t)stream, (const bf16_t*)dy,
                     (const unsigned char*)argmax, (bf16_t*)dx, N, H, W, C, Ho,
                     Wo, lv);
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_gap_fwd(const void* x, void* y, int N, int HW, int C,
                             void* stream) {
  hipLaunchKernelGGL(k_gap_fwd, dim3(N), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, (bf16_t*)y, HW, C);
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_gap_bwd(const void* dy, void* dx, int N, int HW, int C,
                             void* stream) {
  long total = (long)N * HW * (C >> 3);
  hipLaunchKernelGGL(k_gap_bwd, dim3(grid_1d(total)), dim3(256), 0,
                     (hipStream_t)stream, (const bf16_t*)dy, (bf16_t*)dx, HW, C,
                     total);
  DDLW_CHECK_LAUNCH();
}
