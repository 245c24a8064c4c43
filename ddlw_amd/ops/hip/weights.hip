// Weight layouts of the dgrad-as-forward-conv routes, one launch each.
//
// A conv weight is stored bf16, flat [K][R][S][C] (channels_last). The
// stride-1 dgrad runs the forward kernel on [C][R][S][K] with both taps
// reversed; the stride-2 3x3 dgrad runs four parity classes, each a
// [C][nr][ns][K] subset of the taps. Per tap both are a [K][C] -> [C][K]
// transpose between two strided matrices, tiled 64x64 through LDS so that the
// reads (along C) and the writes (along K) are both 16-byte and coalesced.
// Pure data movement: the packed bytes equal what the torch expressions in
// ops/conv_gemm.py produce (tests/test_dgrad_wpack.py).
//
// This file is compiled without packed fp32 arithmetic (build.py).
#include "common.h"

#define WP_TILE 64
#define WP_PITCH 72  // bf16 per LDS row: 144 B, 16-B aligned, breaks the bank stride

// out[c * out_pitch + k] = in[k * in_pitch + c] over the tile at (k0, c0).
// K and C are multiples of 8, so an 8-wide vector is inside or outside as one.
__device__ __forceinline__ void transpose_tile(
    const bf16_t* __restrict__ in, long in_pitch, bf16_t* __restrict__ out,
    long out_pitch, int K, int C, int k0, int c0) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[WP_TILE][WP_PITCH];
  #pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int v = threadIdx.x + i * 256;
    const int row = v >> 3, cv = v & 7;
    const int k = k0 + row, c = c0 + cv * 8;
    if (k < K && c < C)
      *reinterpret_cast<uint4*>(&tile[row][cv * 8]) =
          *reinterpret_cast<const uint4*>(in + (long)k * in_pitch + c);
  }
  __syncthreads();
  #pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int v = threadIdx.x + i * 256;
    const int crow = v >> 3, kv = v & 7;
    const int c = c0 + crow, k = k0 + kv * 8;
    if (c < C && k < K) {
      bf16x8 o;
      #pragma unroll
      for (int j = 0; j < 8; ++j) o.h[j] = tile[kv * 8 + j][crow];
      *reinterpret_cast<uint4*>(out + (long)c * out_pitch + k) = o.v;
    }
  }
}

// grid (ceil(C/64), ceil(K/64), R*S); tap t of the input lands at R*S-1-t
// (both axes reversed)
__global__ __launch_bounds__(256) void k_dgrad_wpack(
    const bf16_t* __restrict__ w, bf16_t* __restrict__ out, int K, int C,
    int RS) {
  const int t = blockIdx.z;
  transpose_tile(w + (long)t * C, (long)RS * C, out + (long)(RS - 1 - t) * K,
                 (long)RS * K, K, C, blockIdx.y * WP_TILE, blockIdx.x * WP_TILE);
}

struct WpackOffs { long v[4]; };

// grid (ceil(C/64), ceil(K/64), 9). Output rows h = 2a + dh take the taps r
// of the parity of h + 1: dh = 0 the tap r = 1, dh = 1 the taps (2, 0) in
// that order; columns alike. Class dh * 2 + dw starts at woffs[class].
__global__ __launch_bounds__(256) void k_dgrad_wpack_s2(
    const bf16_t* __restrict__ w, bf16_t* __restrict__ wcat, int K, int C,
    WpackOffs woffs) {
  const int r = blockIdx.z / 3, s = blockIdx.z % 3;
  const int dh = r != 1, dw = s != 1;
  const int ir = r == 0, is = s == 0;  // position in the class's tap list
  const int nr = dh + 1, ns = dw + 1;
  transpose_tile(w + (long)blockIdx.z * C, 9L * C,
                 wcat + woffs.v[dh * 2 + dw] + (long)(ir * ns + is) * K,
                 (long)nr * ns * K, K, C, blockIdx.y * WP_TILE,
                 blockIdx.x * WP_TILE);
}

static inline const char* wpack_args_bad(int K, int C) {
  if (K < 8 || C < 8 || K % 8 != 0 || C % 8 != 0)
    return "K and C must be positive multiples of 8";
  if (cdiv(K, WP_TILE) > 65535) return "K too large";
  return nullptr;
}

// w bf16 [K][R][S][C] -> out bf16 [C][R][S][K], out[c][r][s][k] =
// w[k][R-1-r][S-1-s][c]
DDLW_EXPORT int ddlw_dgrad_wpack(const void* w, void* out, int K, int C, int R,
                                 int S, void* stream) {
  if (const char* why = wpack_args_bad(K, C)) return ddlw_fail("dgrad_wpack", why);
  if (R < 1 || S < 1 || (long)R * S > 65535)
    return ddlw_fail("dgrad_wpack", "R*S must be in [1, 65535]");
  dim3 grid(cdiv(C, WP_TILE), cdiv(K, WP_TILE), R * S);
  hipLaunchKernelGGL(k_dgrad_wpack, grid, dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)w, (bf16_t*)out, K, C, R * S);
  DDLW_CHECK_LAUNCH();
}

// w bf16 [K][3][3][C] -> wcat: the four parity classes (dh, dw) of the
// stride-2 pad-1 dgrad, class dh * 2 + dw a [C][nr][ns][K] block at element
// offset woffs[class] (host array of 4)
DDLW_EXPORT int ddlw_dgrad_wpack_s2(const void* w, void* wcat, int K, int C,
                                    const long* woffs, void* stream) {
  if (const char* why = wpack_args_bad(K, C)) return ddlw_fail("dgrad_wpack_s2", why);
  WpackOffs o;
  for (int i = 0; i < 4; ++i) {
    if (woffs[i] < 0 || woffs[i] % 8 != 0)
      return ddlw_fail("dgrad_wpack_s2", "class offsets must be non-negative multiples of 8");
    o.v[i] = woffs[i];
  }
  dim3 grid(cdiv(C, WP_TILE), cdiv(K, WP_TILE), 9);
  hipLaunchKernelGGL(k_dgrad_wpack_s2, grid, dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)w, (bf16_t*)wcat, K, C, o);
  DDLW_CHECK_LAUNCH();
}
