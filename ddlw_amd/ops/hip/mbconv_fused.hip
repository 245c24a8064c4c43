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

// ---------------------------------------------------------------------------
// k_mbconv_fused_s2 — the stride-2 block (expand 1x1 -> depthwise 3x3 s2 p1 ->
// project 1x1, no residual) in one kernel; the data contract of
// k_mbconv_fused. Ho = (H - 1) / 2 + 1, Wo likewise.
//   - a workgroup of 4 waves owns a TH x 7 tile of OUTPUT pixels of one image.
//     Its input halo is (2 TH + 1) x 15 pixels from gy = 2 oy0 - 1,
//     gx = 2 ox0 - 1, staged once into LDS like the stride-1 tile (predicated,
//     clamped, mb_xstride). With even H (W) the bottom (right) pad row is
//     never read; with odd H (W) it is, as a zero.
//   - TH = 7 for Cin <= 32: 225 halo pixels as 240 rows (15 fragments), one
//     32-deep expand step. TH = 4 for 32 < Cin <= 96: 135 pixels as 144 rows
//     (9 fragments), 28 output pixels as 32 rows, up to three steps, and two
//     workgroups per image on the 14^2 -> 7^2 layer instead of one.
//   - per 64-channel chunk of the hidden axis:
//       expand   the w1 fragments of the chunk are loaded once. Wave w:
//                channel pair w & 1, the first (w >> 1 == 0) or second half of
//                the pixel fragments (8 | 7 of 15, 5 | 4 of 9), in passes of
//                at most four fragments: 32 accumulator VGPRs beside the
//                project accumulators. Epilogue as at stride 1; a halo pixel
//                outside the image is written to h1 as zero.
//       depthwise output pixel (oy, ox) reads h1[(2 oy + r) * 15 + 2 ox + s];
//                one thread per 8-channel vector of an output pixel, weights,
//                s2, b2 loaded before the barrier -> h2[OROWS][64], rows past
//                the tile zero.
//       project  as at stride 1 over MF = 4 | 2 pixel fragments.
//     The same two barriers per chunk with the same single-buffer argument:
//     the next expand writes h1 only after the "h2 ready" barrier, which ends
//     every depthwise read of h1, and the next depthwise writes h2 only after
//     the next "h1 ready" barrier, which every wave reaches after its project
//     reads of h2.
//   - epilogue s3, b3, 16-byte stores over Ho x Wo masked by pixel and Cout.
// LDS: XROWS * xstride * 2 + XROWS * 144 + OROWS * 144 bytes: 62976 at TH 7,
// Cin 32; 55296 at TH 4, Cin 96. h1 has a row for every staged row, so the
// expand epilogue writes whole fragments (the rows past the halo as zeros).
#define MB2_TW 7                     // output tile width
#define MB2_HW (2 * MB2_TW + 1)      // halo width
#define MB2_MAX_CIN 96

template <int TH>
struct mb2_geom {
  static constexpr int HPIX = (2 * TH + 1) * MB2_HW;  // 225 | 135 halo pixels
  static constexpr int NF = (HPIX + 15) / 16;         // 15 | 9 fragments
  static constexpr int XROWS = NF * 16;
  static constexpr int NFH = (NF + 1) / 2;            // 8 | 5: first half
  static constexpr int NPASS = (NFH + 3) / 4;
  static constexpr int OPIX = TH * MB2_TW;            // 49 | 28 output pixels
  static constexpr int MF = (OPIX + 15) / 16;         // 4 | 2 fragments
  static constexpr int OROWS = MF * 16;
  static constexpr int KS = TH == 7 ? 1 : 3;          // 32-deep expand steps
};

template <int TH, int NPW>
__global__ __launch_bounds__(256) void k_mbconv_fused_s2(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w1,
    const float* __restrict__ s1, const float* __restrict__ b1,
    const bf16_t* __restrict__ wd, const float* __restrict__ s2,
    const float* __restrict__ b2, const bf16_t* __restrict__ w3,
    const float* __restrict__ s3, const float* __restrict__ b3,
    bf16_t* __restrict__ y, int H, int W, int Ho, int Wo, int Cin, int Chid,
    int Cout, int tilesY, int tilesX, int xstride) {
  using G = mb2_geom<TH>;
  extern __shared__ __attribute__((aligned(16))) bf16_t mb_smem[];
  bf16_t* xs = mb_smem;                      // [XROWS][xstride]
  bf16_t* h1 = xs + G::XROWS * xstride;      // [XROWS][MB_HS], rows past HPIX zero
  bf16_t* h2 = h1 + G::XROWS * MB_HS;        // [OROWS][MB_HS]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: uniform branches
  const int l15 = lane & 15;
  const int lg = lane >> 4;
  int blk = blockIdx.x;
  const int tx = blk % tilesX;
  blk /= tilesX;
  const int ty = blk % tilesY;
  const long n = blk / tilesY;
  const int oy0 = ty * TH, ox0 = tx * MB2_TW;
  const int gy0 = 2 * oy0 - 1, gx0 = 2 * ox0 - 1;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  // ---- stage the x halo tile; the rows of h2 past the tile are zero for good ----
  const int cv = Cin >> 3;
  for (int i = tid; i < G::XROWS * cv; i += 256) {
    const int r = i / cv, v = i - r * cv;
    const int hy = r / MB2_HW, hx = r - hy * MB2_HW;
    const int gy = gy0 + hy, gx = gx0 + hx;
    const bool ok = r < G::HPIX && gy >= 0 && gy < H && gx >= 0 && gx < W;
    uint4 val = *reinterpret_cast<const uint4*>(
        x + ((n * H + clamp_tap(gy, H - 1)) * W + clamp_tap(gx, W - 1)) * Cin + v * 8);
    if (!ok) val = zero;
    *reinterpret_cast<uint4*>(xs + r * xstride + v * 8) = val;
  }
  if (tid < (G::OROWS - G::OPIX) * (MB_HS / 8))
    *reinterpret_cast<uint4*>(h2 + G::OPIX * MB_HS + tid * 8) = zero;

  // expand: this wave's channel pair and its half of the pixel fragments
  const int ep = wave & 1;
  const int ef0 = (wave >> 1) * G::NFH;
  const int ef1 = (wave >> 1) ? G::NF : G::NFH;
  u32 inimg = 0;                             // bit j: fragment ef0 + j, row l15
  #pragma unroll
  for (int j = 0; j < G::NPASS * 4; ++j) {
    const int r = (ef0 + j) * 16 + l15;
    const int hy = r / MB2_HW, hx = r - hy * MB2_HW;
    const int gy = gy0 + hy, gx = gx0 + hx;
    if (r < G::HPIX && gy >= 0 && gy < H && gx >= 0 && gx < W) inimg |= 1u << j;
  }
  // depthwise: this thread's channel vector of the chunk
  const int dv = tid & 7;

  mb_f32x4 pacc[NPW][2][G::MF];
  #pragma unroll
  for (int q = 0; q < NPW; ++q)
    #pragma unroll
    for (int f = 0; f < 2; ++f)
      #pragma unroll
      for (int m = 0; m < G::MF; ++m) pacc[q][f][m] = mb_f32x4{0.f, 0.f, 0.f, 0.f};

  __syncthreads();

  for (int hc0 = 0; hc0 < Chid; hc0 += MB_CH) {
    // ---- expand ----
    // keeps the eight bit tests of inimg in the loop: hoisted, they are eight
    // lane masks in SGPR pairs and the NPW = 3 instances run out of SGPRs
    asm volatile("" : "+v"(inimg));
    const int hcb = hc0 + ep * 32 + lg * 8;      // this lane's 8 hidden channels
    const bool hok = hcb < Chid;
    float sc1[8], bi1[8];
    load8f(s1 + (hok ? hcb : 0), sc1);
    load8f(b1 + (hok ? hcb : 0), bi1);
    mb_frag fw[G::KS][2];
    #pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int k = hc0 + ep * 32 + (l15 >> 2) * 8 + f * 4 + (l15 & 3);
      const bool kok = k < Chid;
      const bf16_t* row = w1 + (long)(kok ? k : Chid - 1) * Cin;
      #pragma unroll
      for (int ks = 0; ks < G::KS; ++ks) {
        const int c = ks * 32 + lg * 8;
        const bool cok = c < Cin;
        fw[ks][f].u = *reinterpret_cast<const uint4*>(row + (cok ? c : 0));
        if (!(cok && kok)) fw[ks][f].u = zero;
      }
    }
    #pragma unroll
    for (int p = 0; p < G::NPASS; ++p) {
      if (ef0 + p * 4 >= ef1) break;             // wave-uniform
      mb_f32x4 eacc[2][4];
      #pragma unroll
      for (int f = 0; f < 2; ++f)
        #pragma unroll
        for (int j = 0; j < 4; ++j) eacc[f][j] = mb_f32x4{0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int ks = 0; ks < G::KS; ++ks) {
        if (ks * 32 >= Cin) break;
        const int c = ks * 32 + lg * 8;
        const bool cok = c < Cin;
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int fr = ef0 + p * 4 + j;
          if (fr >= ef1) continue;               // wave-uniform
          mb_frag fx;
          fx.u = *reinterpret_cast<const uint4*>(
              xs + (fr * 16 + l15) * xstride + (cok ? c : 0));
          if (!cok) fx.u = zero;
          #pragma unroll
          for (int f = 0; f < 2; ++f)
            eacc[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                fw[ks][f].v, fx.v, eacc[f][j], 0, 0, 0);
        }
      }
      #pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int fr = ef0 + p * 4 + j;
        const int r = fr * 16 + l15;
        if (fr >= ef1) continue;
        bf16x8 o;
        o.v = zero;
        if (((inimg >> (p * 4 + j)) & 1u) && hok) {
          #pragma unroll
          for (int e = 0; e < 8; ++e)
            o.h[e] = f2b(apply_act(eacc[e >> 2][j][e & 3] * sc1[e] + bi1[e], 2));
        }
        *reinterpret_cast<uint4*>(h1 + r * MB_HS + ep * 32 + lg * 8) = o.v;
      }
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

    // ---- depthwise, stride 2 ----
    for (int pix = tid >> 3; pix < G::OPIX; pix += 32) {
      const int oy = pix / MB2_TW, ox = pix - oy * MB2_TW;
      float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int t = 0; t < 9; ++t) {
        bf16x8 hv, wv;
        hv.v = *reinterpret_cast<const uint4*>(
            h1 + ((2 * oy + t / 3) * MB2_HW + 2 * ox + t % 3) * MB_HS + dv * 8);
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
      mb_frag fh[G::MF];
      #pragma unroll
      for (int m = 0; m < G::MF; ++m)
        fh[m].u = *reinterpret_cast<const uint4*>(
            h2 + (m * 16 + l15) * MB_HS + ks * 32 + lg * 8);
      #pragma unroll
      for (int q = 0; q < NPW; ++q) {
        if ((wave + 4 * q) * 32 >= Cout) continue;   // wave-uniform
        #pragma unroll
        for (int f = 0; f < 2; ++f)
          #pragma unroll
          for (int m = 0; m < G::MF; ++m)
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
    for (int m = 0; m < G::MF; ++m) {
      const int pix = m * 16 + l15;
      const int oy = pix / MB2_TW, ox = pix - oy * MB2_TW;
      const int gy = oy0 + oy, gx = ox0 + ox;
      if (pix >= G::OPIX || gy >= Ho || gx >= Wo) continue;
      bf16x8 o;
      #pragma unroll
      for (int e = 0; e < 8; ++e)
        o.h[e] = f2b(pacc[q][e >> 2][m][e & 3] * sc[e] + bi[e]);
      *reinterpret_cast<uint4*>(y + ((n * Ho + gy) * Wo + gx) * Cout + kb) = o.v;
    }
  }
}

// As ddlw_mbconv_fused_fwd with a stride-2 depthwise and no residual: y is
// [N][(H-1)/2+1][(W-1)/2+1][Cout]. Cin <= 96.
DDLW_EXPORT int ddlw_mbconv_fused_s2_fwd(const void* x, const void* w1, const void* s1,
                                         const void* b1, const void* wd, const void* s2,
                                         const void* b2, const void* w3, const void* s3,
                                         const void* b3, void* y, int N, int H, int W,
                                         int Cin, int Chid, int Cout, void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("mbconv_fused_s2_fwd", why); };
  if (Cin <= 0 || Cin % 8 != 0 || Chid <= 0 || Chid % 8 != 0 || Cout <= 0 ||
      Cout % 8 != 0)
    return fail("Cin, Chid and Cout must be positive multiples of 8");
  if (Cin > MB2_MAX_CIN) return fail("Cin must be at most 96");
  if (Cout > MB_MAX_COUT) return fail("Cout must be at most 320");
  if (N < 0 || H <= 0 || W <= 0) return fail("N, H, W must be positive");
  if (!x || !w1 || !s1 || !b1 || !wd || !s2 || !b2 || !w3 || !s3 || !b3 || !y)
    return fail("null pointer");
  if ((((size_t)x | (size_t)w1 | (size_t)s1 | (size_t)b1 | (size_t)wd |
        (size_t)s2 | (size_t)b2 | (size_t)w3 | (size_t)s3 | (size_t)b3 |
        (size_t)y) & 15) != 0)
    return fail("pointers must be 16-byte aligned");
  if (N == 0) return 0;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int th = Cin <= 32 ? 7 : 4;
  const long tilesY = cdiv(Ho, th), tilesX = cdiv(Wo, MB2_TW);
  const long blocks = (long)N * tilesY * tilesX;
  if (blocks >= (1l << 31)) return fail("grid too large");
  const int xstride = mb_xstride(Cin);
  const int npw = (int)cdiv(cdiv(Cout, 32), 4);  // 1, 2 or 3 pairs per wave
  with_int<7, 4>(th, [&](auto THc) {
    using G = mb2_geom<decltype(THc)::value>;
    const size_t lds = sizeof(bf16_t) *
                       ((size_t)G::XROWS * xstride + G::XROWS * MB_HS + G::OROWS * MB_HS);
    with_int<1, 2, 3>(npw, [&](auto NPc) {
      hipLaunchKernelGGL(
          (k_mbconv_fused_s2<decltype(THc)::value, decltype(NPc)::value>),
          dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream,
          (const bf16_t*)x, (const bf16_t*)w1, (const float*)s1, (const float*)b1,
          (const bf16_t*)wd, (const float*)s2, (const float*)b2, (const bf16_t*)w3,
          (const float*)s3, (const float*)b3, (bf16_t*)y, H, W, Ho, Wo, Cin, Chid,
          Cout, (int)tilesY, (int)tilesX, xstride);
    });
  });
  DDLW_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// k_dwpw_fused — the t = 1 block (depthwise 3x3 s1 p1 + ReLU6 -> project 1x1,
// + residual) in one kernel:
//   h2 = relu6(dw3x3(x; wd) * s2 + b2)          rounded to bf16
//   y  =       (h2 * w3^T) * s3 + b3 (+ x)      one rounding to bf16
// There is no expand: the staged x halo IS the depthwise input, zero padding
// is on x itself. Per pixel the work is tiny and the kernel is memory-bound:
//   - a workgroup of 4 waves owns a 14x14 tile of output pixels of one image
//     (112, 56, 28, 14 are multiples of 14); its 16x16 halo (1.31x the tile)
//     is staged once into LDS, predicated and clamped, row stride mb_xstride.
//     One barrier in the whole kernel.
//   - C <= 64 is one chunk and Cout <= 64 at most two 32-channel pairs, so
//     the waves split the 13 PIXEL fragments of the project (wave, wave + 4,
//     ...), not Cout. h2 never exists in memory, not even in LDS: lane
//     (l15, lg) of a B fragment holds channels 32 ks + 8 lg .. + 7 of pixel
//     16 fr + l15, so each lane computes the depthwise of exactly that vector
//     (nine taps from the LDS halo, fp32, weights in registers for the whole
//     kernel) and rounds it into its MFMA operand register. A pixel row past
//     the tile reads pixel 195's taps (in bounds) and is masked at the store;
//     a pixel is a column of the MFMA, so it touches no other pixel.
//   - w3 fragments (<= 8), s3, b3 stay in registers for the whole kernel; the
//     residual is the centre of the LDS halo. Channel tails (C, Cout not a
//     multiple of 32) are zero fragments from clamped loads.
// KS = 32-deep steps over C, NP = 32-channel pairs of Cout: 1 or 2 each.
// LDS: 256 * xstride * 2 bytes: 20480 at C 32, 36864 at C 64.
#define DP_T 14
#define DP_HALO (DP_T + 2)
#define DP_HPIX (DP_HALO * DP_HALO)  // 256 halo pixels
#define DP_OPIX (DP_T * DP_T)        // 196 output pixels
#define DP_NF ((DP_OPIX + 15) / 16)  // ... as 13 fragments
#define DP_MAX_C 64

template <int KS, int NP, bool HAS_RES>
__global__ __launch_bounds__(256) void k_dwpw_fused(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ wd,
    const float* __restrict__ s2, const float* __restrict__ b2,
    const bf16_t* __restrict__ w3, const float* __restrict__ s3,
    const float* __restrict__ b3, bf16_t* __restrict__ y, int H, int W, int C,
    int Cout, int tilesY, int tilesX, int xstride) {
  extern __shared__ __attribute__((aligned(16))) bf16_t mb_smem[];
  bf16_t* xs = mb_smem;                      // [256][xstride]

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
  const int y0 = ty * DP_T, x0 = tx * DP_T;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  // ---- stage the x halo tile ----
  const int cv = C >> 3;
  for (int i = tid; i < DP_HPIX * cv; i += 256) {
    const int r = i / cv, v = i - r * cv;
    const int gy = y0 - 1 + r / DP_HALO, gx = x0 - 1 + r % DP_HALO;
    const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
    uint4 val = *reinterpret_cast<const uint4*>(
        x + ((n * H + clamp_tap(gy, H - 1)) * W + clamp_tap(gx, W - 1)) * C + v * 8);
    if (!ok) val = zero;
    *reinterpret_cast<uint4*>(xs + r * xstride + v * 8) = val;
  }

  // ---- this lane's operands, in flight over the barrier ----
  uint4 wt[KS][9];
  float sc2[KS][8], bi2[KS][8];
  int chl[KS];
  bool vok[KS];
  #pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int ch = ks * 32 + lg * 8;         // this lane's 8 channels of step ks
    vok[ks] = ch < C;
    chl[ks] = vok[ks] ? ch : 0;
    #pragma unroll
    for (int t = 0; t < 9; ++t)
      wt[ks][t] = *reinterpret_cast<const uint4*>(wd + (long)t * C + chl[ks]);
    load8f(s2 + chl[ks], sc2[ks]);
    load8f(b2 + chl[ks], bi2[ks]);
  }
  mb_frag fw3[KS][NP][2];
  float sc3[NP][8], bi3[NP][8];
  #pragma unroll
  for (int q = 0; q < NP; ++q) {
    #pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int k = q * 32 + (l15 >> 2) * 8 + f * 4 + (l15 & 3);
      const bf16_t* row = w3 + (long)(k < Cout ? k : Cout - 1) * C;
      #pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        fw3[ks][q][f].u = *reinterpret_cast<const uint4*>(row + chl[ks]);
        if (!(vok[ks] && k < Cout)) fw3[ks][q][f].u = zero;
      }
    }
    const int kb = q * 32 + lg * 8;
    load8f(s3 + (kb < Cout ? kb : 0), sc3[q]);
    load8f(b3 + (kb < Cout ? kb : 0), bi3[q]);
  }
  __syncthreads();

  for (int fr = wave; fr < DP_NF; fr += 4) {
    const int pix = fr * 16 + l15;
    const int pc = pix < DP_OPIX ? pix : DP_OPIX - 1;
    const int oy = pc / DP_T, ox = pc - oy * DP_T;
    // ---- depthwise, straight into the B fragments ----
    mb_frag fh[KS];
    #pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int t = 0; t < 9; ++t) {
        bf16x8 hv, wv;
        hv.v = *reinterpret_cast<const uint4*>(
            xs + ((oy + t / 3) * DP_HALO + ox + t % 3) * xstride + chl[ks]);
        wv.v = wt[ks][t];
        #pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += b2f(hv.h[e]) * b2f(wv.h[e]);
      }
      bf16x8 o;
      o.v = zero;
      if (vok[ks]) {
        #pragma unroll
        for (int e = 0; e < 8; ++e)
          o.h[e] = f2b(apply_act(a[e] * sc2[ks][e] + bi2[ks][e], 2));
      }
      fh[ks].u = o.v;
    }
    // ---- project + epilogue ----
    const int gy = y0 + oy, gx = x0 + ox;
    const bool pok = pix < DP_OPIX && gy < H && gx < W;
    #pragma unroll
    for (int q = 0; q < NP; ++q) {
      mb_f32x4 acc[2] = {mb_f32x4{0.f, 0.f, 0.f, 0.f}, mb_f32x4{0.f, 0.f, 0.f, 0.f}};
      #pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        #pragma unroll
        for (int f = 0; f < 2; ++f)
          acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              fw3[ks][q][f].v, fh[ks].v, acc[f], 0, 0, 0);
      const int kb = q * 32 + lg * 8;
      if (!pok || kb >= Cout) continue;
      float v[8];
      #pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = acc[e >> 2][e & 3] * sc3[q][e] + bi3[q][e];
      if constexpr (HAS_RES) {                   // C == Cout: kb < C
        bf16x8 r;
        r.v = *reinterpret_cast<const uint4*>(
            xs + ((oy + 1) * DP_HALO + ox + 1) * xstride + kb);
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

// x [N][H][W][C], wd [9][C], w3 [Cout][C], y [N][H][W][Cout] bf16; s2, b2 fp32
// [C]; s3, b3 fp32 [Cout]; res: add x to the output (needs C == Cout).
DDLW_EXPORT int ddlw_dwpw_fused_fwd(const void* x, const void* wd, const void* s2,
                                    const void* b2, const void* w3, const void* s3,
                                    const void* b3, void* y, int N, int H, int W, int C,
                                    int Cout, int res, void* stream) {
  auto fail = [](const char* why) { return ddlw_fail("dwpw_fused_fwd", why); };
  if (C <= 0 || C % 8 != 0 || Cout <= 0 || Cout % 8 != 0)
    return fail("C and Cout must be positive multiples of 8");
  if (C > DP_MAX_C || Cout > DP_MAX_C) return fail("C and Cout must be at most 64");
  if (res != 0 && C != Cout) return fail("the residual needs C == Cout");
  if (N < 0 || H <= 0 || W <= 0) return fail("N, H, W must be positive");
  if (!x || !wd || !s2 || !b2 || !w3 || !s3 || !b3 || !y) return fail("null pointer");
  if ((((size_t)x | (size_t)wd | (size_t)s2 | (size_t)b2 | (size_t)w3 | (size_t)s3 |
        (size_t)b3 | (size_t)y) & 15) != 0)
    return fail("pointers must be 16-byte aligned");
  if (N == 0) return 0;
  const long tilesY = cdiv(H, DP_T), tilesX = cdiv(W, DP_T);
  const long blocks = (long)N * tilesY * tilesX;
  if (blocks >= (1l << 31)) return fail("grid too large");
  const int xstride = mb_xstride(C);
  const size_t lds = sizeof(bf16_t) * (size_t)DP_HPIX * xstride;
  with_int<1, 2>((int)cdiv(C, 32), [&](auto KSc) {
    with_int<1, 2>((int)cdiv(Cout, 32), [&](auto NPc) {
      with_bool(res != 0, [&](auto HR) {
        hipLaunchKernelGGL(
            (k_dwpw_fused<decltype(KSc)::value, decltype(NPc)::value,
                          decltype(HR)::value>),
            dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream,
            (const bf16_t*)x, (const bf16_t*)wd, (const float*)s2, (const float*)b2,
            (const bf16_t*)w3, (const float*)s3, (const float*)b3, (bf16_t*)y, H, W,
            C, Cout, (int)tilesY, (int)tilesX, xstride);
      });
    });
  });
  DDLW_CHECK_LAUNCH();
}
