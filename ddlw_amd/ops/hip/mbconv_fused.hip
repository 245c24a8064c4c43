// Frozen MobileNetV2 inverted residual (expand 1x1 -> depthwise 3x3 s1 p1 ->
// project 1x1, every BN folded, + residual) in ONE kernel. NHWC bf16 in/out,
// fp32 accumulation:
//   h1 = relu6((x  * w1^T) * s1 + b1)           rounded to bf16
//   h2 = relu6(dw3x3(h1; wd)  * s2 + b2)        rounded to bf16
//   y  =       (h2 * w3^T) * s3 + b3 (+ x)      one rounding to bf16
// h1 and h2 are rounded where pw_conv_fwd / depthwise_fwd_ep / pw_conv_fwd
// round them, so this is the function the three-kernel path computes; they
// exist only in LDS. One launch instead of three, and none of the four
// passes over the 6x-wide hidden tensor.
//
// k_mbconv_fused — work split and data movement:
//   - a workgroup of 4 waves owns one 7x7 tile of output pixels of one image
//     (112, 56, 28, 14, 7 are all multiples of 7); grid N * ceil(H/7) *
//     ceil(W/7), partial tiles masked at the store.
//   - its 9x9 = 81-pixel input halo is staged once into LDS as 96 rows (six
//     16-row MFMA fragments; rows 81..95 zero). Halo pixels outside the image
//     are loaded from a clamped in-bounds address and zeroed (the predicated
//     staging of pointwise.hip). The row stride is an odd number of 16-byte
//     units, so the fragment reads spread over the banks. The centre 7x7 of
//     the tile is the residual.
//   - the hidden axis goes in chunks of 64 channels. Per chunk:
//       expand   [96 x Cin] * [Cin x 64] on v_mfma_f32_16x16x32_bf16, w1 as
//                the A operand straight from global in the PW_TILE_MMA row
//                order (k = 8*(i>>2) + 4*f + (i&3): a lane ends with 8
//                consecutive hidden channels of one pixel), x fragments from
//                LDS. Wave w: channel pair w&1, pixel fragments 3*(w>>1)..+2.
//                Epilogue s1, b1, ReLU6 -> bf16 -> LDS h1[81][64]. A halo
//                pixel outside the image is written as ZERO, not relu6(b1):
//                the depthwise conv pads the hidden tensor, not x.
//       depthwise one thread per 8-channel vector of an output pixel (its
//                vector is the same for both of its pixels, so the 9 weight
//                vectors and s2, b2 are loaded once per chunk), nine taps from
//                LDS in fp32 -> bf16 -> LDS h2[64][64], rows 49..63 zero.
//       project  [64 x 64] * [64 x Cout] accumulated in fp32 registers that
//                live across the chunk loop. The waves split Cout by
//                32-channel pairs (pair w, w+4, w+8), so no cross-wave
//                reduction; w3 fragments are loaded from global before the
//                depthwise stage and used after it.
//     Two barriers per chunk (h1 ready, h2 ready). h1 is rewritten by the
//     next expand only after the barrier that ended its depthwise reads, and
//     h2 by the next depthwise only after the next "h1 ready" barrier, which
//     every wave reaches after its project reads: single buffers suffice and
//     a wave's next expand overlaps the other waves' project.
//   - a Chid tail (whole 8-channel vectors, Chid % 8 == 0): w1 rows, w3
//     columns, h1 and h2 vectors past Chid are zero, scale/bias/weight loads
//     clamped in bounds: the tail contributes exactly zero.
//   - epilogue s3, b3, residual from the LDS x tile, 16-byte stores masked by
//     pixel validity and Cout. No atomics; two calls are bit-equal.
// LDS: 96 * xstride * 2 (<= 32256 B at Cin 160) + 11664 (h1) + 9216 (h2).
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 mb_bf16x8;
typedef __attribute__((ext_vector_type(4))) float mb_f32x4;

#define MB_T 7                       // output tile edge
#define MB_HALO (MB_T + 2)           // halo edge
#define MB_HPIX (MB_HALO * MB_HALO)  // 81 halo pixels
#define MB_XROWS 96                  // ... staged as six 16-row fragments
#define MB_OPIX (MB_T * MB_T)        // 49 output pixels
#define MB_OROWS 64                  // ... as four fragments
#define MB_CH 64                     // hidden channels per chunk
#define MB_HS (MB_CH + 8)            // h1 / h2 row stride: 9 x 16 B
#define MB_MAX_CIN 160
#define MB_MAX_COUT 320

// x-tile row stride in bf16: Cin plus padding to an odd count of 16-byte units
static inline int mb_xstride(int Cin) {
  const int v = Cin / 8 + 1;
  return (v | 1) * 8;
}

union mb_frag {
  uint4 u;
  mb_bf16x8 v;
};

template <int NPW, bool HAS_RES>
__global__ __launch_bounds__(256) void k_mbconv_fused(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w1,
    const float* __restrict__ s1, const float* __restrict__ b1,
    const bf16_t* __restrict__ wd, const float* __restrict__ s2,
    const float* __restrict__ b2, const bf16_t* __restrict__ w3,
    const float* __restrict__ s3, const float* __restrict__ b3,
    bf16_t* __restrict__ y, int H, int W, int Cin, int Chid, int Cout,
    int tilesY, int tilesX, int xstride) {
  extern __shared__ __attribute__((aligned(16))) bf16_t mb_smem[];
  bf16_t* xs = mb_smem;                      // [96][xstride]
  bf16_t* h1 = xs + MB_XROWS * xstride;      // [81][MB_HS]
  bf16_t* h2 = h1 + MB_HPIX * MB_HS;         // [64][MB_HS]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l15 = lane & 15;
  const int lg = lane >> 4;
  int blk = blockIdx.x;
  const int tx = blk % tilesX;
  blk /= tilesX;
  const int ty = blk % tilesY;
  const long n = blk / tilesY;
  const int y0 = ty * MB_T, x0 = tx * MB_T;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  // ---- stage the x halo tile; rows 49..63 of h2 are zero for good ----
  const int cv = Cin >> 3;
  for (int i = tid; i < MB_XROWS * cv; i += 256) {
    const int r = i / cv, v = i - r * cv;
    const int hy = r / MB_HALO, hx = r - hy * MB_HALO;
    const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
    const bool ok = r < MB_HPIX && gy >= 0 && gy < H && gx >= 0 && gx < W;
    uint4 val = *reinterpret_cast<const uint4*>(
        x + ((n * H + clamp_tap(gy, H - 1)) * W + clamp_tap(gx, W - 1)) * Cin + v * 8);
    if (!ok) val = zero;
    *reinterpret_cast<uint4*>(xs + r * xstride + v * 8) = val;
  }
  if (tid < (MB_OROWS - MB_OPIX) * (MB_HS / 8))
    *reinterpret_cast<uint4*>(h2 + MB_OPIX * MB_HS + tid * 8) = zero;

  // expand: this wave's channel pair and its three pixel fragments
  const int ep = wave & 1;
  const int epf0 = (wave >> 1) * 3;
  bool inimg[3];
  #pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int r = (epf0 + j) * 16 + l15;
    const int hy = r / MB_HALO, hx = r - hy * MB_HALO;
    const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
    inimg[j] = r < MB_HPIX && gy >= 0 && gy < H && gx >= 0 && gx < W;
  }
  // depthwise: this thread's channel vector of the chunk
  const int dv = tid & 7;

  mb_f32x4 pacc[NPW][2][4];
  #pragma unroll
  for (int q = 0; q < NPW; ++q)
    #pragma unroll
    for (int f = 0; f < 2; ++f)
      #pragma unroll
      for (int m = 0; m < 4; ++m) pacc[q][f][m] = mb_f32x4{0.f, 0.f, 0.f, 0.f};

  __syncthreads();

  for (int hc0 = 0; hc0 < Chid; hc0 += MB_CH) {
    // ---- expand ----
    const int hcb = hc0 + ep * 32 + lg * 8;      // this lane's 8 hidden channels
    const bool hok = hcb < Chid;
    float sc1[8], bi1[8];
    load8f(s1 + (hok ? hcb : 0), sc1);
    load8f(b1 + (hok ? hcb : 0), bi1);
    const bf16_t* w1row[2];
    bool w1ok[2];
    #pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int k = hc0 + ep * 32 + (l15 >> 2) * 8 + f * 4 + (l15 & 3);
      w1ok[f] = k < Chid;
      w1row[f] = w1 + (long)(w1ok[f] ? k : Chid - 1) * Cin;
    }
    mb_f32x4 eacc[2][3];
    #pragma unroll
    for (int f = 0; f < 2; ++f)
      #pragma unroll
      for (int j = 0; j < 3; ++j) eacc[f][j] = mb_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < Cin; c0 += 32) {
      const int c = c0 + lg * 8;
      const bool cok = c < Cin;
      const int cc = cok ? c : 0;
      mb_frag fw[2], fx[3];
      #pragma unroll
      for (int f = 0; f < 2; ++f) {
        fw[f].u = *reinterpret_cast<const uint4*>(w1row[f] + cc);
        if (!(cok && w1ok[f])) fw[f].u = zero;
      }
      #pragma unroll
      for (int j = 0; j < 3; ++j) {
        fx[j].u = *reinterpret_cast<const uint4*>(
            xs + ((epf0 + j) * 16 + l15) * xstride + cc);
        if (!cok) fx[j].u = zero;
      }
      #pragma unroll
      for (int f = 0; f < 2; ++f)
        #pragma unroll
        for (int j = 0; j < 3; ++j)
          eacc[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              fw[f].v, fx[j].v, eacc[f][j], 0, 0, 0);
    }
    #pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int r = (epf0 + j) * 16 + l15;
      if (r >= MB_HPIX) continue;
      bf16x8 o;
      o.v = zero;
      if (inimg[j] && hok) {
        #pragma unroll
        for (int e = 0; e < 8; ++e)
          o.h[e] = f2b(apply_act(eacc[e >> 2][j][e & 3] * sc1[e] + bi1[e], 2));
      }
      *reinterpret_cast<uint4*>(h1 + r * MB_HS + ep * 32 + lg * 8) = o.v;
    }

    // depthwise operands and the project weights: in flight over the barrier
    const int hcv = hc0 + dv * 8;
    const bool vok = hcv < Chid;
    const int hcl = vok ? hcv : 0;
    uint4 wt[9];
    #pragma unroll
    for (int t = 0; t < 9; ++t)
      wt[t] = *reinterpret_cast<const uint4*>(wd + (long)t * Chid + hcl);
    float sc2[8], bi2[8];
    load8f(s2 + hcl, sc2);
    load8f(b2 + hcl, bi2);
    mb_frag fw3[MB_CH / 32][NPW][2];
    #pragma unroll
    for (int ks = 0; ks < MB_CH / 32; ++ks) {
      const int col = hc0 + ks * 32 + lg * 8;
      const bool cok = col < Chid;
      #pragma unroll
      for (int q = 0; q < NPW; ++q)
        #pragma unroll
        for (int f = 0; f < 2; ++f) {
          const int k = (wave + 4 * q) * 32 + (l15 >> 2) * 8 + f * 4 + (l15 & 3);
          const bool ok = cok && k < Cout;
          fw3[ks][q][f].u = *reinterpret_cast<const uint4*>(
              w3 + (long)(k < Cout ? k : Cout - 1) * Chid + (cok ? col : 0));
          if (!ok) fw3[ks][q][f].u = zero;
        }
    }
    __syncthreads();                             // h1 ready

    // ---- depthwise ----
    for (int pix = tid >> 3; pix < MB_OPIX; pix += 32) {
      const int oy = pix / MB_T, ox = pix - oy * MB_T;
      float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int t = 0; t < 9; ++t) {
        bf16x8 hv, wv;
        hv.v = *reinterpret_cast<const uint4*>(
            h1 + ((oy + t / 3) * MB_HALO + ox + t % 3) * MB_HS + dv * 8);
        wv.v = wt[t];
        #pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += b2f(hv.h[e]) * b2f(wv.h[e]);
      }
      bf16x8 o;
      o.v = zero;
      if (vok) {
        #pragma unroll
        for (int e = 0; e < 8; ++e)
          o.h[e] = f2b(apply_act(a[e] * sc2[e] + bi2[e], 2));
      }
      *reinterpret_cast<uint4*>(h2 + pix * MB_HS + dv * 8) = o.v;
    }
    __syncthreads();                             // h2 ready

    // ---- project ----
    #pragma unroll
    for (int ks = 0; ks < MB_CH / 32; ++ks) {
      if (hc0 + ks * 32 >= Chid) break;
      mb_frag fh[4];
      #pragma unroll
      for (int m = 0; m < 4; ++m)
        fh[m].u = *reinterpret_cast<const uint4*>(
            h2 + (m * 16 + l15) * MB_HS + ks * 32 + lg * 8);
      #pragma unroll
      for (int q = 0; q < NPW; ++q) {
        if ((wave + 4 * q) * 32 >= Cout) continue;   // wave-uniform
        #pragma unroll
        for (int f = 0; f < 2; ++f)
          #pragma unroll
          for (int m = 0; m < 4; ++m)
            pacc[q][f][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                fw3[ks][q][f].v, fh[m].v, pacc[q][f][m], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: lane (lg, l15) holds channels kb..kb+7 of pixel m*16+l15 ----
  #pragma unroll
  for (int q = 0; q < NPW; ++q) {
    const int kb = (wave + 4 * q) * 32 + lg * 8;
    if (kb >= Cout) continue;
    float sc[8], bi[8];
    load8f(s3 + kb, sc);
    load8f(b3 + kb, bi);
    #pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int pix = m * 16 + l15;
      const int oy = pix / MB_T, ox = pix - oy * MB_T;
      const int gy = y0 + oy, gx = x0 + ox;
      if (pix >= MB_OPIX || gy >= H || gx >= W) continue;
      float v[8];
      #pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = pacc[q][e >> 2][m][e & 3] * sc[e] + bi[e];
      if constexpr (HAS_RES) {                   // Cin == Cout: kb < Cin
        bf16x8 r;
        r.v = *reinterpret_cast<const uint4*>(
            xs + ((oy + 1) * MB_HALO + ox + 1) * xstride + kb);
        #pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += b2f(r.h[e]);
      }
      bf16x8 o;
      #pragma unroll
      for (int e = 0; e < 8; ++e) o.h[e] = f2b(v[e]);
      *reinterpret_cast<uint4*>(y + ((n * H + gy) * W + gx) * Cout + kb) = o.v;
    }
  }
}

// x [N][H][W][Cin], w1 [Chid][Cin], wd [9][Chid], w3 [Cout][Chid], y
// [N][H][W][Cout] bf16; s1, b1, s2, b2 fp32 [Chid]; s3, b3 fp32 [Cout]; res:
// add x to the output (needs Cin == Cout). Stride 1, pad 1.
DDLW_EXPORT int ddlw_mbconv_fused_fwd(const void* x, const void* w1, const void* s1,
                                      const void* b1, const void* wd, const void* s2,
                                      const void* b2, const void* w3, const void* s3,
                                      const void* b3, void* y, int N, int H, int W,
                                      int Cin, int Chid, int Cout, int res,
                                      void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("mbconv_fused_fwd", why); };
  if (Cin <= 0 || Cin % 8 != 0 || Chid <= 0 || Chid % 8 != 0 || Cout <= 0 ||
      Cout % 8 != 0)
    return fail("Cin, Chid and Cout must be positive multiples of 8");
  if (Cin > MB_MAX_CIN) return fail("Cin must be at most 160");
  if (Cout > MB_MAX_COUT) return fail("Cout must be at most 320");
  if (res != 0 && Cin != Cout) return fail("the residual needs Cin == Cout");
  if (N < 0 || H <= 0 || W <= 0) return fail("N, H, W must be positive");
  if (!x || !w1 || !s1 || !b1 || !wd || !s2 || !b2 || !w3 || !s3 || !b3 || !y)
    return fail("null pointer");
  if ((((size_t)x | (size_t)w1 | (size_t)s1 | (size_t)b1 | (size_t)wd |
        (size_t)s2 | (size_t)b2 | (size_t)w3 | (size_t)s3 | (size_t)b3 |
        (size_t)y) & 15) != 0)
    return fail("pointers must be 16-byte aligned");
  if (N == 0) return 0;
  const long tilesY = cdiv(H, MB_T), tilesX = cdiv(W, MB_T);
  const long blocks = (long)N * tilesY * tilesX;
  if (blocks >= (1l << 31)) return fail("grid too large");
  const int xstride = mb_xstride(Cin);
  const size_t lds = sizeof(bf16_t) *
                     ((size_t)MB_XROWS * xstride + MB_HPIX * MB_HS + MB_OROWS * MB_HS);
  const int npw = (int)cdiv(cdiv(Cout, 32), 4);  // 1, 2 or 3 pairs per wave
  with_int<1, 2, 3>(npw, [&](auto NPc) {
    with_bool(res != 0, [&](auto HR) {
      hipLaunchKernelGGL(
          (k_mbconv_fused<decltype(NPc)::value, decltype(HR)::value>),
          dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream,
          (const bf16_t*)x, (const bf16_t*)w1, (const float*)s1, (const float*)b1,
          (const bf16_t*)wd, (const float*)s2, (const float*)b2, (const bf16_t*)w3,
          (const float*)s3, (const float*)b3, (bf16_t*)y, H, W, Cin, Chid, Cout,
          (int)tilesY, (int)tilesX, xstride);
    });
  });
  DDLW_CHECK_LAUNCH();
}
