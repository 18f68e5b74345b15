// The FID Inception-v3 feature extractor (pytorch-fid's InceptionV3 with use_fid_inception=True, the port of the TF FID graph),
// inference only, NHWC fp32:
//
//   incep_conv     conv + folded BatchNorm + ReLU as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
//                  accumulation): M = B Ho Wo pixels, N = Co, K = R S Ci in (r, s, ci) order; separate strides and pads per
//                  axis; the input read from a channel slice (ctot_in, c0_in) and the output written into a channel slice
//                  (ctot_out, c0_out) of the block's concatenated tensor
//   incep_pool3    3 x 3 pools: max stride 2 pad 0, max stride 1 pad 1, average stride 1 pad 1 without the pad in the divisor
//   incep_gap      global average pool [B, H W, C] -> [B, C], pixels summed in order
//   incep_prep     NCHW or NHWC [B, 3, H, W] -> NHWC [B, Ho, Wo, 4]: bilinear resize (align_corners=False), a x + b, channel 3 = 0
//
// Every output element is computed by one thread or one workgroup in a fixed order that does not depend on the batch size (no
// split-K, no atomics): reruns are bit-identical and an image's features do not depend on the other images of its batch.
#include "common.h"

namespace diagan {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- implicit-GEMM convolution ----------------------------------------------------------------------------------------------
// 128 pixels x 64 output channels per workgroup, K in steps of 16 through LDS; 4 waves in a 2 (pixels) x 2 (channels) grid, each
// wave 64 x 32 = two 32 x 32 accumulators.  MFMA 32x32x2 f32 operands: A[row = lane & 31][k = lane >> 5] (a pixel),
// B[k = lane >> 5][col = lane & 31] (a channel); result register e of lane l is C[row = 4 (l >> 5) + (e & 3) + 8 (e >> 2)][col = l & 31].
// The next K-step's global loads are held in registers while the current one is multiplied.
constexpr int IC_BM = 128, IC_BN = 64, IC_BK = 16, IC_T = 256;
constexpr int IC_LDA = IC_BM + 4, IC_LDB = IC_BN + 4;   // row strides 16 banks apart: the four k-groups of a store land apart

struct IncepConvArgs {
  const float* x;
  const float* w;      // [Co][Kp], k = (r S + s) Ci + ci, zero for k >= R S Ci
  const float* bias;   // [Co]
  float* y;
  int B, H, W, ctot_in, c0_in, Ci;
  int Co, R, S, Kp, sh, sw, ph, pw;
  int Ho, Wo, ctot_out, c0_out, relu;
};

__global__ __launch_bounds__(IC_T) void incep_conv_kernel(const IncepConvArgs a) {
  __shared__ float As[IC_BK][IC_LDA];   // As[k][m]: im2col rows of the tile's pixels
  __shared__ float Bs[IC_BK][IC_LDB];   // Bs[k][n]: the folded weights
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int M = a.B * a.Ho * a.Wo, K = a.R * a.S * a.Ci;
  const int m0 = blockIdx.x * IC_BM, n0 = blockIdx.y * IC_BN;
  const int kg = tid & 3;               // this thread's k-group of 4 in every K-step (A and B)

  // the two pixels this thread gathers (tile rows (tid >> 2) and (tid >> 2) + 64), decoded once
  const float* xb[2];
  int iy0[2], ix0[2];
  bool pv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int p = m0 + (tid >> 2) + 64 * j;
    pv[j] = p < M;
    const int pp = pv[j] ? p : 0;
    const int b = pp / (a.Ho * a.Wo), rem = pp - b * (a.Ho * a.Wo);
    const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
    iy0[j] = oy * a.sh - a.ph;
    ix0[j] = ox * a.sw - a.pw;
    xb[j] = a.x + (long)b * a.H * a.W * a.ctot_in + a.c0_in;
  }
  const int wn_row = n0 + (tid >> 2);   // this thread's weight row
  const float* wrow = a.w + (long)(wn_row < a.Co ? wn_row : 0) * a.Kp;

  f32x4 ra[2], rb;
  auto load = [&](int k0) {
    const int k = k0 + 4 * kg;
    int r = 0, s = 0, ci = 0;
    const bool kv = k < K;
    if (kv) {
      const int rs = k / a.Ci;
      ci = k - rs * a.Ci;
      r = rs / a.S;
      s = rs - r * a.S;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int iy = iy0[j] + r, ix = ix0[j] + s;
      const bool v = kv && pv[j] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      ra[j] = v ? *reinterpret_cast<const f32x4*>(xb[j] + ((long)iy * a.W + ix) * a.ctot_in + ci) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    rb = wn_row < a.Co ? *reinterpret_cast<const f32x4*>(wrow + k) : f32x4{0.f, 0.f, 0.f, 0.f};   // k < Kp always
  };
  auto store = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) As[4 * kg + e][(tid >> 2) + 64 * j] = ra[j][e];
#pragma unroll
    for (int e = 0; e < 4; ++e) Bs[4 * kg + e][tid >> 2] = rb[e];
  };

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  const int fi = lane & 31, fh = lane >> 5;
  const int wm = (w & 1) * 64, wn = (w >> 1) * 32;
  load(0);
  for (int k0 = 0; k0 < a.Kp; k0 += IC_BK) {
    store();
    __syncthreads();
    if (k0 + IC_BK < a.Kp) load(k0 + IC_BK);
#pragma unroll
    for (int s = 0; s < IC_BK / 2; ++s) {
      const int kr = 2 * s + fh;
      const float b = Bs[kr][wn + fi];
      const float a0 = As[kr][wm + fi], a1 = As[kr][wm + 32 + fi];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
    }
    __syncthreads();
  }

  const int ch = n0 + wn + fi;
  if (ch >= a.Co) return;
  const float bv = a.bias[ch];
  float* yc = a.y + a.c0_out + ch;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int p = m0 + wm + 32 * i + 4 * fh + (e & 3) + 8 * (e >> 2);
      if (p < M) {
        float v = acc[i][e] + bv;
        if (a.relu) v = fmaxf(v, 0.f);
        yc[(long)p * a.ctot_out] = v;
      }
    }
}

// ---- 3 x 3 pools ------------------------------------------------------------------------------------------------------------
// one thread per (output pixel, 4 channels); taps in (dy, dx) order; pad taps are skipped (max) or left out of the divisor (avg)
__global__ __launch_bounds__(256) void incep_pool3_kernel(const float* __restrict__ x, int B, int H, int W, int ctot_in, int c0_in,
                                                          int C, float* __restrict__ y, int Ho, int Wo, int ctot_out, int c0_out,
                                                          int stride, int pad, int avg) {
  const int C4 = C >> 2;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)B * Ho * Wo * C4;
  if (idx >= total) return;
  const int c = (int)(idx % C4) * 4;
  const long p = idx / C4;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), b = (int)(p / ((long)Wo * Ho));
  const float* xb = x + (long)b * H * W * ctot_in + c0_in + c;
  f32x4 r = avg ? f32x4{0.f, 0.f, 0.f, 0.f} : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int n = 0;
  for (int dy = 0; dy < 3; ++dy) {
    const int iy = oy * stride - pad + dy;
    if (iy < 0 || iy >= H) continue;
    for (int dx = 0; dx < 3; ++dx) {
      const int ix = ox * stride - pad + dx;
      if (ix < 0 || ix >= W) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(xb + ((long)iy * W + ix) * ctot_in);
      if (avg) {
        r += v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = fmaxf(r[e], v[e]);
      }
      ++n;
    }
  }
  if (avg) r = r / (float)n;
  *reinterpret_cast<f32x4*>(y + p * ctot_out + c0_out + c) = r;
}

// ---- global average pool ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void incep_gap_kernel(const float* __restrict__ x, int B, int HW, int C, float* __restrict__ y) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * C) return;
  const int b = (int)(idx / C), c = (int)(idx % C);
  const float* xb = x + (long)b * HW * C + c;
  float s = 0.f;
  for (int i = 0; i < HW; ++i) s += xb[(long)i * C];
  y[idx] = s / (float)HW;
}

// ---- input prep -------------------------------------------------------------------------------------------------------------
// torch's upsample_bilinear2d (align_corners=False, no antialias): src = (dst + 0.5) in / out - 0.5 clamped at 0, the upper
// neighbour clamped at the last row / column
__global__ __launch_bounds__(256) void incep_prep_kernel(const float* __restrict__ x, int nhwc, int B, int H, int W,
                                                         float* __restrict__ y, int Ho, int Wo, int resize, float sa, float sb) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (long)B * Ho * Wo) return;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), b = (int)(p / ((long)Wo * Ho));
  const long cs = nhwc ? 1 : (long)H * W, ps = nhwc ? 3 : 1;   // channel and pixel strides
  const float* xb = x + (long)b * 3 * H * W;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (!resize) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = sa * xb[c * cs + ((long)oy * W + ox) * ps] + sb;
  } else {
    // source coordinates and weights in float64: in fp32 the weight's rounding grows with the coordinate (2.6e-5 at 256 -> 299)
    const double sy = fmax((double)H / Ho * (oy + 0.5) - 0.5, 0.0), sx = fmax((double)W / Wo * (ox + 0.5) - 0.5, 0.0);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly1 = (float)(sy - y0), ly0 = (float)(1.0 - (sy - y0)), lx1 = (float)(sx - x0), lx0 = (float)(1.0 - (sx - x0));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* xc = xb + c * cs;
      const float v = ly0 * (lx0 * xc[((long)y0 * W + x0) * ps] + lx1 * xc[((long)y0 * W + x1) * ps]) +
                      ly1 * (lx0 * xc[((long)y1 * W + x0) * ps] + lx1 * xc[((long)y1 * W + x1) * ps]);
      o[c] = sa * v + sb;
    }
  }
  *reinterpret_cast<f32x4*>(y + p * 4) = o;
}

}  // namespace diagan

using namespace diagan;

DIAGAN_API int diagan_incep_conv_kp(int R, int S, int Ci) {
  if (R <= 0 || S <= 0 || Ci <= 0) return set_err(DIAGAN_EINVAL, "incep_conv_kp: bad geometry %d x %d x %d", R, S, Ci);
  const long K = (long)R * S * Ci;
  return (int)((K + IC_BK - 1) / IC_BK * IC_BK);
}

DIAGAN_API int diagan_incep_conv(const float* x, int B, int H, int W, int ctot_in, int c0_in, int Ci, const float* w,
                                 const float* bias, int Co, int R, int S, int Kp, int stride_h, int stride_w, int pad_h, int pad_w,
                                 float* y, int Ho, int Wo, int ctot_out, int c0_out, int relu, void* stream) {
  DG_REQUIRE(x && w && bias && y, "incep_conv: NULL pointer");
  DG_REQUIRE(B > 0 && H > 0 && W > 0 && Ci > 0 && Co > 0 && R > 0 && S > 0 && stride_h > 0 && stride_w > 0 && pad_h >= 0 &&
                 pad_w >= 0, "incep_conv: bad geometry");
  DG_REQUIRE(Ci % 4 == 0 && ctot_in % 4 == 0 && c0_in % 4 == 0 && c0_in >= 0 && c0_in + Ci <= ctot_in,
             "incep_conv: input slice [%d, %d) of %d channels (multiples of 4 needed)", c0_in, c0_in + Ci, ctot_in);
  DG_REQUIRE(c0_out >= 0 && c0_out + Co <= ctot_out, "incep_conv: output slice [%d, %d) of %d channels", c0_out, c0_out + Co,
             ctot_out);
  DG_REQUIRE(Kp == diagan_incep_conv_kp(R, S, Ci), "incep_conv: Kp %d, expected %d", Kp, diagan_incep_conv_kp(R, S, Ci));
  DG_REQUIRE(Ho == (H + 2 * pad_h - R) / stride_h + 1 && Wo == (W + 2 * pad_w - S) / stride_w + 1 && Ho > 0 && Wo > 0,
             "incep_conv: output %d x %d does not match the geometry", Ho, Wo);
  DG_REQUIRE((long)B * Ho * Wo < (1L << 31) && (long)B * H * W * ctot_in < (1L << 40), "incep_conv: too large");
  DG_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0,
             "incep_conv: x and w must be 16-byte aligned");
  IncepConvArgs a{x, w, bias, y, B, H, W, ctot_in, c0_in, Ci, Co, R, S, Kp, stride_h, stride_w, pad_h, pad_w, Ho, Wo, ctot_out,
                  c0_out, relu ? 1 : 0};
  const long M = (long)B * Ho * Wo;
  incep_conv_kernel<<<dim3(cdiv(M, IC_BM), cdiv(Co, IC_BN)), IC_T, 0, (hipStream_t)stream>>>(a);
  return check_launch("incep_conv");
}

DIAGAN_API int diagan_incep_pool3(const float* x, int B, int H, int W, int ctot_in, int c0_in, int C, float* y, int Ho, int Wo,
                                  int ctot_out, int c0_out, int mode, void* stream) {
  DG_REQUIRE(x && y && x != y, "incep_pool3: NULL or aliased pointer");
  DG_REQUIRE(mode >= 0 && mode <= 2, "incep_pool3: mode %d (0 max s2 p0, 1 max s1 p1, 2 avg s1 p1 without the pad)", mode);
  DG_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "incep_pool3: bad geometry");
  DG_REQUIRE(C % 4 == 0 && ctot_in % 4 == 0 && c0_in % 4 == 0 && ctot_out % 4 == 0 && c0_out % 4 == 0 && c0_in >= 0 &&
                 c0_out >= 0 && c0_in + C <= ctot_in && c0_out + C <= ctot_out,
             "incep_pool3: channel slices must be in range and multiples of 4");
  DG_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0,
             "incep_pool3: x and y must be 16-byte aligned");
  const int stride = mode == 0 ? 2 : 1, pad = mode == 0 ? 0 : 1;
  DG_REQUIRE(Ho == (H + 2 * pad - 3) / stride + 1 && Wo == (W + 2 * pad - 3) / stride + 1 && Ho > 0 && Wo > 0,
             "incep_pool3: output %d x %d does not match the geometry", Ho, Wo);
  const long n = (long)B * Ho * Wo * (C / 4);
  incep_pool3_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(x, B, H, W, ctot_in, c0_in, C, y, Ho, Wo, ctot_out, c0_out,
                                                                   stride, pad, mode == 2);
  return check_launch("incep_pool3");
}

DIAGAN_API int diagan_incep_gap(const float* x, int B, int HW, int C, float* y, void* stream) {
  DG_REQUIRE(x && y, "incep_gap: NULL pointer");
  DG_REQUIRE(B > 0 && HW > 0 && C > 0, "incep_gap: bad geometry");
  incep_gap_kernel<<<cdiv((long)B * C, 256), 256, 0, (hipStream_t)stream>>>(x, B, HW, C, y);
  return check_launch("incep_gap");
}

DIAGAN_API int diagan_incep_prep(const float* x, int nhwc, int B, int H, int W, float* y, int Ho, int Wo, int resize, float a,
                                 float b, void* stream) {
  DG_REQUIRE(x && y, "incep_prep: NULL pointer");
  DG_REQUIRE(B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "incep_prep: bad geometry");
  DG_REQUIRE(resize || (Ho == H && Wo == W), "incep_prep: without resize the output is the input's size");
  DG_REQUIRE((reinterpret_cast<uintptr_t>(y) & 15) == 0, "incep_prep: y must be 16-byte aligned");
  const long n = (long)B * Ho * Wo;
  incep_prep_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(x, nhwc ? 1 : 0, B, H, W, y, Ho, Wo, resize ? 1 : 0, a, b);
  return check_launch("incep_prep");
}
