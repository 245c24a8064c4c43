// What the pointwise (1x1) GEMM kernels share: the MFMA fragment types, the
// wave/block tile of k_pw_conv's geometry and its choice of NP
// (pointwise.hip, pointwise_frozen.hip).
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 pw_bf16x8;
typedef __attribute__((ext_vector_type(4))) float pw_f32x4;

#define PW_MR 2                    // 16-row fragments per wave
#define PW_WAVES 4
#define PW_BM (PW_WAVES * PW_MR * 16)

// 32-channel fragment pairs per wave: the smallest listed NP that covers K in
// one tile, else whichever of 5 / 6 wastes fewer pairs over ceil(K/32).
static inline int pw_pick_np(int K) {
  const int kp = (K + 31) / 32;
  if (kp <= 3) return kp;
  if (kp <= 5) return 5;
  if (kp == 6) return 6;
  const int w5 = (kp + 4) / 5 * 5, w6 = (kp + 5) / 6 * 6;
  return w5 < w6 ? 5 : 6;
}
