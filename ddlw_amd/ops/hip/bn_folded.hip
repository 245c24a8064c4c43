// Fold + finalize of a LARGE BatchNorm partial set in one launch.
//
// The conv epilogues hand over up to ~12k partial rows. bn.hip reduces them in
// two launches: k_bn_parts_fold (chip-filling grid, nparts -> G stage rows),
// then k_bn_finalize / k_bn_grad_finalize (ceil(C/32) blocks, G rows -> the
// result). Here the second launch is the tail of the first: every block folds
// its stage row exactly as k_bn_parts_fold does and draws a ticket from the
// integer counter of its channel group (blockIdx.x); the block that draws
// ticket G - 1 knows that all G stage rows of its group are written and
// finishes exactly as the finalize kernel does. No block waits for another:
// there is no spin and no inter-block barrier, a block that is not last just
// exits. The only atomic is the integer ticket; every floating-point sum is
// taken in the two-kernel path's order, term for term, so the results are
// bit-equal to it (tests/test_bn_folded.py).
//
// Visibility of the stage rows across the XCDs (one L2 each): every thread
// issues __threadfence() (an agent-scope fence) after its stage stores and
// before the block barrier that precedes the ticket; the ticket itself is an
// agent-scope acq_rel __hip_atomic_fetch_add; the last block issues
// __threadfence() again before it reads the stage rows. The stage pointers
// are neither const nor __restrict__: the kernel reads what other blocks of
// the same launch wrote.
//
// The counters are zero between launches: the last block of a channel group
// stores 0 to its counter when it is done. Launches that share a counter
// buffer must be ordered (one buffer per stream, ops/runtime.py).
//
// Summation order. The loops of bn.hip's three kernels are compiled (fast
// math, packed fp32) to TWO interleaved accumulators: terms 0, 2, 4, ... and
// terms 1, 3, 5, ... of a thread's strided partial list are summed apart, the
// two sums are added, and an odd last term comes on top; a list of one term is
// 0 + term. The tail of k_bn_finalize is compiled to reciprocals, one fused
// multiply-add for the variance and one for running_var, and
// momentum * unbiased as (var * (rows * momentum)) / (rows - 1). This file is
// compiled without packed fp32 arithmetic (build.py), so the compiler would
// choose another order here; the order above is therefore written out, and
// reassociation and contraction are switched off for the whole file so that it
// stands as written. The back end still fuses under fast math whatever the
// pragma says ((1 - momentum) * x became x - momentum * x), so the products of
// the running-stat update are pinned in registers (pin) before they are added.
#include "common.h"

#pragma clang fp reassociate(off) contract(off)

// the value as it stands in a VGPR: nothing is folded across this point
__device__ __forceinline__ float pin(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// (sum of a[p * C + c], sum of b[p * C + c]) over p = p0, p0 + step, ... < end,
// in the two-accumulator order described above
__device__ __forceinline__ void strided_sum2(const float* a, const float* b,
                                             long p0, long step, long end,
                                             int C, int c, float& s, float& q) {
  s = 0.f;
  q = 0.f;
  if (p0 >= end) return;
  const long n = (end - p0 + step - 1) / step;
  const long n2 = n & ~1L;
  long p = p0;
  if (n2 != 0) {
    float s1 = 0.f, q1 = 0.f;
    for (long i = 0; i < n2; i += 2, p += 2 * step) {
      s += a[p * C + c];
      s1 += a[(p + step) * C + c];
      q += b[p * C + c];
      q1 += b[(p + step) * C + c];
    }
    s += s1;
    q += q1;
  }
  if (n2 != n) {
    s += a[p * C + c];
    q += b[p * C + c];
  }
}

// k_bn_parts_fold's body on block (blockIdx.x, blockIdx.y), then the ticket.
// True in the one block per channel group that drew the last ticket.
__device__ __forceinline__ bool fold_then_ticket(
    const float* __restrict__ ps, const float* __restrict__ pq, float* os,
    float* oq, int* ticket, long nparts, int C, int G, float (*ls)[32],
    float (*lq)[32]) {
  const int cl = threadIdx.x & 31;
  const int pg = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const int g = blockIdx.y;
  float s = 0.f, q = 0.f;
  if (c < C) strided_sum2(ps, pq, (long)g * 8 + pg, (long)G * 8, nparts, C, c, s, q);
  ls[pg][cl] = s;
  lq[pg][cl] = q;
  __syncthreads();
  if (pg == 0 && c < C) {
    #pragma unroll
    for (int i = 1; i < 8; ++i) {
      s += ls[i][cl];
      q += lq[i][cl];
    }
    os[(long)g * C + c] = s;
    oq[(long)g * C + c] = q;
  }
  __threadfence();  // release the stage row at agent scope
  __shared__ int last;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = __hip_atomic_fetch_add(ticket + blockIdx.x, 1, __ATOMIC_ACQ_REL,
                                         __HIP_MEMORY_SCOPE_AGENT);
    last = (t == G - 1);
  }
  __syncthreads();  // also: ls / lq are free for the second tree
  if (!last) return false;
  __threadfence();  // acquire the other blocks' stage rows
  return true;
}

__device__ __forceinline__ void ticket_reset(int* ticket) {
  if (threadIdx.x == 0)
    __hip_atomic_store(ticket + blockIdx.x, 0, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_bn_finalize_folded(
    const float* __restrict__ ps, const float* __restrict__ pq,
    float* stage_sum, float* stage_sumsq, int* ticket,
    float* __restrict__ mean, float* __restrict__ rstd,
    float* __restrict__ running_mean, float* __restrict__ running_var,
    long rows, int C, long nparts, int G, float eps, float momentum) {
  __shared__ float ls[8][32], lq[8][32];
  if (!fold_then_ticket(ps, pq, stage_sum, stage_sumsq, ticket, nparts, C, G,
                        ls, lq))
    return;
  // k_bn_finalize over the G stage rows
  const int cl = threadIdx.x & 31;
  const int pg = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float s = 0.f, q = 0.f;
  if (c < C) strided_sum2(stage_sum, stage_sumsq, pg, 8, G, C, c, s, q);
  ls[pg][cl] = s;
  lq[pg][cl] = q;
  __syncthreads();
  if (pg == 0 && c < C) {
    #pragma unroll
    for (int g = 1; g < 8; ++g) {
      s += ls[g][cl];
      q += lq[g][cl];
    }
    const float rowsf = (float)rows;
    const float inv_rows = __builtin_amdgcn_rcpf(rowsf);
    const float m = s * inv_rows;
    const float var = fmaxf(__builtin_fmaf(-m, m, q * inv_rows), 0.f);
    mean[c] = m;
    rstd[c] = rsqrtf(var + eps);
    if (running_mean) {
      const float inv_rows1 =
          __builtin_amdgcn_rcpf((float)(rows > 1 ? rows - 1 : 1));
      const float keep = pin(1.f - momentum);
      const float km = pin(keep * running_mean[c]);
      const float mm = pin(momentum * m);
      running_mean[c] = km + mm;
      const float kv = pin(keep * running_var[c]);
      const float mv = pin(var * pin(rowsf * momentum));
      running_var[c] = __builtin_fmaf(inv_rows1, mv, kv);
    }
  }
  ticket_reset(ticket);
}

__global__ __launch_bounds__(256) void k_bn_grad_finalize_folded(
    const float* __restrict__ pdb, const float* __restrict__ pdg,
    float* stage_db, float* stage_dg, int* ticket, float* __restrict__ dbeta,
    float* __restrict__ dgamma, int C, long nparts, int G) {
  __shared__ float lb[8][32], lg[8][32];
  if (!fold_then_ticket(pdb, pdg, stage_db, stage_dg, ticket, nparts, C, G,
                        lb, lg))
    return;
  // k_bn_grad_finalize over the G stage rows
  const int cl = threadIdx.x & 31;
  const int pg = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float b = 0.f, g = 0.f;
  if (c < C) strided_sum2(stage_db, stage_dg, pg, 8, G, C, c, b, g);
  lb[pg][cl] = b;
  lg[pg][cl] = g;
  __syncthreads();
  if (pg == 0 && c < C) {
    #pragma unroll
    for (int gg = 1; gg < 8; ++gg) {
      b += lb[gg][cl];
      g += lg[gg][cl];
    }
    dbeta[c] = b;
    dgamma[c] = g;
  }
  ticket_reset(ticket);
}

// ---------------------------------------------------------------------------
// launchers. stage: fp32 [2][G][C]; ticket: nticket ints, all zero, shared by
// the launches of one stream only.
// ---------------------------------------------------------------------------
static inline const char* folded_args_bad(int C, long nparts, int G,
                                          int nticket) {
  if (C < 1 || nparts < 1) return "C and nparts must be positive";
  if (G < 1 || G > 65535) return "G must be in [1, 65535]";
  if ((C + 31) / 32 > nticket) return "ticket buffer smaller than ceil(C/32)";
  return nullptr;
}

DDLW_EXPORT int ddlw_bn_finalize_folded(const void* part_sum,
                                        const void* part_sumsq, void* stage,
                                        void* ticket, int nticket, void* mean,
                                        void* rstd, void* rmean, void* rvar,
                                        long rows, int C, long nparts, int G,
                                        float eps, float momentum,
                                        void* stream) {
  if (const char* why = folded_args_bad(C, nparts, G, nticket))
    return ddlw_fail("bn_finalize_folded", why);
  float* st = (float*)stage;
  hipLaunchKernelGGL(k_bn_finalize_folded, dim3((C + 31) / 32, G), dim3(256),
                     0, (hipStream_t)stream, (const float*)part_sum,
                     (const float*)part_sumsq, st, st + (long)G * C,
                     (int*)ticket, (float*)mean, (float*)rstd, (float*)rmean,
                     (float*)rvar, rows, C, nparts, G, eps, momentum);
  DDLW_CHECK_LAUNCH();
}

DDLW_EXPORT int ddlw_bn_grad_finalize_folded(const void* part_db,
                                             const void* part_dg, void* stage,
                                             void* ticket, int nticket,
                                             void* dbeta, void* dgamma, int C,
                                             long nparts, int G,
                                             void* stream) {
  if (const char* why = folded_args_bad(C, nparts, G, nticket))
    return ddlw_fail("bn_grad_finalize_folded", why);
  float* st = (float*)stage;
  hipLaunchKernelGGL(k_bn_grad_finalize_folded, dim3((C + 31) / 32, G),
                     dim3(256), 0, (hipStream_t)stream, (const float*)part_db,
                     (const float*)part_dg, st, st + (long)G * C, (int*)ticket,
                     (float*)dbeta, (float*)dgamma, C, nparts, G);
  DDLW_CHECK_LAUNCH();
}
