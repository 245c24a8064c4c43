// Multi-tensor fused optimizers: one launch steps every parameter through a
// device-resident descriptor array. fp32 master weights and state, fp32 or
// bf16 grads, optional bf16 shadow of the weights. grid.y walks the chunks,
// grid.x (capped at 512) strides over the largest one.
#include "common.h"

// ---------------------------------------------------------------------------
// Fused SGD (momentum + weight decay + nesterov-free), multi-tensor (K10 /
// "fused SGD step" in the BASELINE north star). Descriptor array of
// {param fp32, grad fp32, momentum fp32, numel} chunks lives in device mem.
// Optional bf16 shadow copy of the weights (model weights in bf16 while the
// master stays fp32).
// ---------------------------------------------------------------------------
struct SgdChunk {
  float* p;        // fp32 master
  const void* g;   // grad: fp32, or bf16 when (flags & 1)
  float* m;        // momentum fp32
  bf16_t* p_bf16;  // nullable bf16 shadow of the weights (the model's param)
  long n;
  long flags;      // bit0: grad is bf16
};

__global__ __launch_bounds__(256) void k_fused_sgd(
    const SgdChunk* __restrict__ chunks, int nchunks,
    float lr, float momentum, float weight_decay, int first_step) {
  for (int ci = blockIdx.y; ci < nchunks; ci += gridDim.y) {
    SgdChunk ch = chunks[ci];
    const bool g_bf16 = ch.flags & 1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < ch.n;
         i += (long)gridDim.x * blockDim.x) {
      float gr = g_bf16 ? b2f(((const bf16_t*)ch.g)[i])
                        : ((const float*)ch.g)[i];
      float g = gr + weight_decay * ch.p[i];
      float v = first_step ? g : momentum * ch.m[i] + g;
      ch.m[i] = v;
      float p = ch.p[i] - lr * v;
      ch.p[i] = p;
      if (ch.p_bf16) ch.p_bf16[i] = f2b(p);
    }
  }
}

DDLW_EXPORT int ddlw_fused_sgd(const void* chunks, int nchunks, long max_numel,
                               float lr, float momentum, float weight_decay,
                               int first_step, void* stream) {
  dim3 grid(grid_1d(max_numel, 256, 512), min(nchunks, 64));
  hipLaunchKernelGGL(k_fused_sgd, grid, dim3(256), 0, (hipStream_t)stream,
                     (const SgdChunk*)chunks, nchunks, lr, momentum,
                     weight_decay, first_step);
  DDLW_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// Fused Adam (K10 — the reference's optimizer, Adam 1e-3; P1/02:201).
// fp32 master path like SGD: m/v/master fp32, optional bf16 param shadow,
// grads fp32 or bf16. Bias correction folded into the step size host-side?
// No — step count varies per call; computed in-kernel from step_t.
// ---------------------------------------------------------------------------
struct AdamChunk {
  float* p;        // fp32 master
  const void* g;   // grad (fp32, or bf16 when flags & 1)
  float* m;        // first moment
  float* v;        // second moment
  bf16_t* p_bf16;  // nullable bf16 shadow
  long n;
  long flags;
};

__global__ __launch_bounds__(256) void k_fused_adam(
    const AdamChunk* __restrict__ chunks, int nchunks, float lr, float beta1,
    float beta2, float eps, float weight_decay, float bc1, float bc2) {
  // bc1 = 1/(1-beta1^t), bc2 = 1/(1-beta2^t) precomputed host-side
  for (int ci = blockIdx.y; ci < nchunks; ci += gridDim.y) {
    AdamChunk ch = chunks[ci];
    const bool g_bf16 = ch.flags & 1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < ch.n;
         i += (long)gridDim.x * blockDim.x) {
      float g = g_bf16 ? b2f(((const bf16_t*)ch.g)[i])
                       : ((const float*)ch.g)[i];
      g += weight_decay * ch.p[i];
      float m = beta1 * ch.m[i] + (1.f - beta1) * g;
      float v = beta2 * ch.v[i] + (1.f - beta2) * g * g;
      ch.m[i] = m;
      ch.v[i] = v;
      float mh = m * bc1;
      float vh = v * bc2;
      float p = ch.p[i] - lr * mh / (sqrtf(vh) + eps);
      ch.p[i] = p;
      if (ch.p_bf16) ch.p_bf16[i] = f2b(p);
    }
  }
}

DDLW_EXPORT int ddlw_fused_adam(const void* chunks, int nchunks, long max_numel,
                                float lr, float beta1, float beta2, float eps,
                                float weight_decay, float bc1, float bc2,
                                void* stream) {
  dim3 grid(grid_1d(max_numel, 256, 512), min(nchunks, 64));
  hipLaunchKernelGGL(k_fused_adam, grid, dim3(256), 0, (hipStream_t)stream,
                     (const AdamChunk*)chunks, nchunks, lr, beta1, beta2, eps,
                     weight_decay, bc1, bc2);
  DDLW_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// Fused Adadelta (K10 — the other optimizer of the reference's HPO space,
// hp.choice('optimizer', ['Adadelta', 'Adam']); P2/01:195). Same layout as
// Adam: fp32 master, square_avg and acc_delta, optional bf16 param shadow,
// grads fp32 or bf16. The update is a ratio of two running RMS values and is
// often far below one bf16 ulp of the weight, so all of it stays in fp32.
// ---------------------------------------------------------------------------
struct AdadeltaChunk {
  float* p;        // fp32 master
  const void* g;   // grad (fp32, or bf16 when flags & 1)
  float* sq;       // running average of g^2
  float* acc;      // running average of delta^2
  bf16_t* p_bf16;  // nullable bf16 shadow
  long n;
  long flags;
};

__global__ __launch_bounds__(256) void k_fused_adadelta(
    const AdadeltaChunk* __restrict__ chunks, int nchunks, float lr, float rho,
    float eps, float weight_decay) {
  for (int ci = blockIdx.y; ci < nchunks; ci += gridDim.y) {
    AdadeltaChunk ch = chunks[ci];
    const bool g_bf16 = ch.flags & 1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < ch.n;
         i += (long)gridDim.x * blockDim.x) {
      float g = g_bf16 ? b2f(((const bf16_t*)ch.g)[i])
                       : ((const float*)ch.g)[i];
      float p = ch.p[i];
      g += weight_decay * p;
      float sq = rho * ch.sq[i] + (1.f - rho) * g * g;
      float acc = ch.acc[i];
      float delta = sqrtf(acc + eps) / sqrtf(sq + eps) * g;
      ch.sq[i] = sq;
      ch.acc[i] = rho * acc + (1.f - rho) * delta * delta;
      p -= lr * delta;
      ch.p[i] = p;
      if (ch.p_bf16) ch.p_bf16[i] = f2b(p);
    }
  }
}

DDLW_EXPORT int ddlw_fused_adadelta(const void* chunks, int nchunks,
                                    long max_numel, float lr, float rho,
                                    float eps, float weight_decay,
                                    void* stream) {
  dim3 grid(grid_1d(max_numel, 256, 512), min(nchunks, 64));
  hipLaunchKernelGGL(k_fused_adadelta, grid, dim3(256), 0, (hipStream_t)stream,
                     (const AdadeltaChunk*)chunks, nchunks, lr, rho, eps,
                     weight_decay);
  DDLW_CHECK_LAUNCH();
}
