// The head of the SimpleConvNet group classifier (the diagan_cls_* part of include/diagan_lpips.h states the contracts).
//
//   cls_head_fwd_kernel    a workgroup per image.  The C / 4 channel groups of a pixel are read by neighbouring lanes in 16-byte
//                          loads; the 256 lanes form R = 256 / (C / 4) rows, row r walks the pixels r, r + R, ... and keeps
//                          four sums of max(scale x + shift, 0).  The rows' sums meet in LDS and are added in row order, then
//                          scaled by 1 / HW: `pooled`.  Wave v forms the logits v, v + 4, ... (lanes stride the channels, the
//                          shuffle butterfly), wave 0 the norm in float64 and `feat`.
//   cls_head_g_kernel      a workgroup per image and run of pixels: the C values (1 / HW) sum_n dlogit[b][n] w[n][c] are formed
//                          once, n ascending, and stored to every pixel of the run -- the same arithmetic in every workgroup of
//                          an image, so the gradient is the same bits at every pixel.
//   cls_head_wgrad_kernel  a lane per element of gw (and of gb): the sum over the batch in row order.
//   cls_histogram_kernel   one workgroup; 256 rows at a time leave their first maximum's column in LDS, lane n counts the
//                          column n; lane n alone reads and writes counts[n].
//
// No atomics; every sum's order is fixed by the shapes.  Products and sums are written as fmaf, one rounding each.
#include "common.h"
#include "diagan_lpips.h"

#include <algorithm>

namespace diagan {

using cl4 = __attribute__((ext_vector_type(4))) float;

constexpr int CL_T = 256;
constexpr int CL_MAX_C = 1024;
constexpr int CL_MAX_N = 64;
constexpr int CL_G_PIXELS = 64;        // pixels a workgroup of the data gradient stores

__global__ __launch_bounds__(CL_T) void cls_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, const float* __restrict__ w,
                                                            const float* __restrict__ bias, int HW, int C, int N,
                                                            float* __restrict__ pooled, float* __restrict__ logits,
                                                            float* __restrict__ feat) {
  __shared__ cl4 part[CL_T];             // [row][channel group]
  __shared__ float pool[CL_MAX_C];
  const int b = blockIdx.x, t = threadIdx.x;
  const int cg = C >> 2, R = CL_T / cg;  // cg <= 256, so R >= 1
  const int r = t / cg, q = t - r * cg;
  if (r < R) {
    const cl4 sc = *reinterpret_cast<const cl4*>(scale + 4 * q), sh = *reinterpret_cast<const cl4*>(shift + 4 * q);
    const float* xp = x + (int64_t)b * HW * C + 4 * q;
    cl4 acc = cl4{0.f, 0.f, 0.f, 0.f};
    for (int p = r; p < HW; p += R) {
      const cl4 v = *reinterpret_cast<const cl4*>(xp + (int64_t)p * C);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += fmaxf(fmaf(sc[e], v[e], sh[e]), 0.f);
    }
    part[r * cg + q] = acc;
  }
  __syncthreads();
  const float inv_hw = 1.f / (float)HW;
  for (int c = t; c < C; c += CL_T) {
    float s = 0.f;
    for (int rr = 0; rr < R; ++rr) s += part[rr * cg + (c >> 2)][c & 3];
    s *= inv_hw;
    pool[c] = s;
    pooled[(int64_t)b * C + c] = s;
  }
  __syncthreads();
  const int lane = t & 63, wave = t >> 6;
  if (logits != nullptr) {
    for (int n = wave; n < N; n += CL_T / 64) {
      float s = 0.f;
      for (int c = lane; c < C; c += 64) s = fmaf(pool[c], w[(int64_t)n * C + c], s);
      s = wave_sum(s);
      if (lane == 0) logits[(int64_t)b * N + n] = s + bias[n];
    }
  }
  if (feat != nullptr && wave == 0) {
    double ss = 0.0;
    for (int c = lane; c < C; c += 64) ss += (double)pool[c] * (double)pool[c];
    ss = wave_sum(ss);
    const double den = fmax(sqrt(ss), 1e-12);
    for (int c = lane; c < C; c += 64) feat[(int64_t)b * C + c] = (float)((double)pool[c] / den);
  }
}

__global__ __launch_bounds__(CL_T) void cls_head_g_kernel(const float* __restrict__ dlogit, const float* __restrict__ w, int HW,
                                                          int C, int N, float* __restrict__ g) {
  __shared__ float v[CL_MAX_C];
  const int b = blockIdx.y, t = threadIdx.x;
  const float inv_hw = 1.f / (float)HW;
  for (int c = t; c < C; c += CL_T) {
    float s = 0.f;
    for (int n = 0; n < N; ++n) s = fmaf(dlogit[(int64_t)b * N + n], w[(int64_t)n * C + c], s);
    v[c] = s * inv_hw;
  }
  __syncthreads();
  const int cg = C >> 2;
  const int p0 = blockIdx.x * CL_G_PIXELS;
  const int np = min(CL_G_PIXELS, HW - p0);
  float* gp = g + ((int64_t)b * HW + p0) * C;
  for (int i = t; i < np * cg; i += CL_T) {
    const int q = i % cg;
    *reinterpret_cast<cl4*>(gp + (int64_t)i * 4) = cl4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  }
}

__global__ __launch_bounds__(CL_T) void cls_head_wgrad_kernel(const float* __restrict__ dlogit, const float* __restrict__ pooled,
                                                              int B, int C, int N, float* __restrict__ gw,
                                                              float* __restrict__ gb) {
  const int i = blockIdx.x * CL_T + threadIdx.x;
  if (gw != nullptr && i < N * C) {
    const int n = i / C, c = i - n * C;
    float s = 0.f;
    int b = 0;
    for (; b + 8 <= B; b += 8) {                     // eight rows' loads in flight; the products are added in row order
      float d[8], p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) d[u] = dlogit[(int64_t)(b + u) * N + n], p[u] = pooled[(int64_t)(b + u) * C + c];
#pragma unroll
      for (int u = 0; u < 8; ++u) s = fmaf(d[u], p[u], s);
    }
    for (; b < B; ++b) s = fmaf(dlogit[(int64_t)b * N + n], pooled[(int64_t)b * C + c], s);
    gw[i] = s;
  }
  if (gb != nullptr && i < N) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dlogit[(int64_t)b * N + i];
    gb[i] = s;
  }
}

__global__ __launch_bounds__(CL_T) void cls_histogram_kernel(const float* __restrict__ logits, int M, int N,
                                                             int64_t* __restrict__ counts) {
  __shared__ int arg[CL_T];
  const int t = threadIdx.x;
  int64_t mine = 0;
  for (int m0 = 0; m0 < M; m0 += CL_T) {
    const int m = m0 + t;
    int a = -1;
    if (m < M) {
      const float* z = logits + (int64_t)m * N;
      float zmax = z[0];
      a = 0;
      for (int n = 1; n < N; ++n)
        if (z[n] > zmax) zmax = z[n], a = n;             // only a greater value replaces the maximum: the first one wins
    }
    arg[t] = a;
    __syncthreads();
    if (t < N) {
      const int rows = min(CL_T, M - m0);
      for (int k = 0; k < rows; ++k) mine += arg[k] == t ? 1 : 0;
    }
    __syncthreads();
  }
  if (t < N) counts[t] += mine;
}

static bool cl_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace diagan

using namespace diagan;

DIAGAN_API int diagan_cls_head_fwd(const float* x, const float* scale, const float* shift, const float* w, const float* bias, int B,
                                   int HW, int C, int N, float* pooled, float* logits, float* feat, void* stream) {
  DG_REQUIRE(x != nullptr && scale != nullptr && shift != nullptr && pooled != nullptr, "diagan_cls_head_fwd: null pointer");
  DG_REQUIRE(logits == nullptr || (w != nullptr && bias != nullptr), "diagan_cls_head_fwd: the logits need w and bias");
  DG_REQUIRE(B >= 1 && HW >= 1 && C >= 4 && C % 4 == 0 && C <= CL_MAX_C && N >= 1 && N <= CL_MAX_N,
             "diagan_cls_head_fwd: bad shape B=%d HW=%d C=%d N=%d (C a multiple of 4 up to %d, N in [1, %d])", B, HW, C, N, CL_MAX_C,
             CL_MAX_N);
  DG_REQUIRE(cl_aligned16(x) && cl_aligned16(scale) && cl_aligned16(shift), "diagan_cls_head_fwd: x, scale and shift must be 16-byte aligned");
  hipLaunchKernelGGL(cls_head_fwd_kernel, dim3(B), dim3(CL_T), 0, (hipStream_t)stream, x, scale, shift, w, bias, HW, C, N, pooled,
                     logits, feat);
  return check_launch("diagan_cls_head_fwd");
}

DIAGAN_API int diagan_cls_head_bwd(const float* dlogit, const float* w, const float* pooled, int B, int HW, int C, int N, float* g,
                                   float* gw, float* gb, void* stream) {
  DG_REQUIRE(dlogit != nullptr, "diagan_cls_head_bwd: null pointer");
  DG_REQUIRE(g == nullptr || w != nullptr, "diagan_cls_head_bwd: g needs w");
  DG_REQUIRE(gw == nullptr || pooled != nullptr, "diagan_cls_head_bwd: gw needs pooled");
  DG_REQUIRE(B >= 1 && HW >= 1 && C >= 4 && C % 4 == 0 && C <= CL_MAX_C && N >= 1 && N <= CL_MAX_N,
             "diagan_cls_head_bwd: bad shape B=%d HW=%d C=%d N=%d (C a multiple of 4 up to %d, N in [1, %d])", B, HW, C, N, CL_MAX_C,
             CL_MAX_N);
  DG_REQUIRE(B <= 65535, "diagan_cls_head_bwd: B=%d is more than 65535 grid rows", B);
  DG_REQUIRE(g == nullptr || cl_aligned16(g), "diagan_cls_head_bwd: g must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (g != nullptr) {
    hipLaunchKernelGGL(cls_head_g_kernel, dim3((HW + CL_G_PIXELS - 1) / CL_G_PIXELS, B), dim3(CL_T), 0, s, dlogit, w, HW, C, N, g);
    const int rc = check_launch("diagan_cls_head_bwd (g)");
    if (rc != DIAGAN_OK) return rc;
  }
  if (gw != nullptr || gb != nullptr) {
    const int items = gw != nullptr ? N * C : N;
    hipLaunchKernelGGL(cls_head_wgrad_kernel, dim3((items + CL_T - 1) / CL_T), dim3(CL_T), 0, s, dlogit, pooled, B, C, N, gw, gb);
    return check_launch("diagan_cls_head_bwd (gw)");
  }
  return DIAGAN_OK;
}

DIAGAN_API int diagan_cls_histogram(const float* logits, int M, int N, int64_t* counts, void* stream) {
  DG_REQUIRE(logits != nullptr && counts != nullptr, "diagan_cls_histogram: null pointer");
  DG_REQUIRE(M >= 1 && N >= 1 && N <= CL_MAX_N, "diagan_cls_histogram: bad shape M=%d N=%d (N <= %d)", M, N, CL_MAX_N);
  DG_REQUIRE(((uintptr_t)counts & 7) == 0, "diagan_cls_histogram: counts must be 8-byte aligned");
  hipLaunchKernelGGL(cls_histogram_kernel, dim3(1), dim3(CL_T), 0, (hipStream_t)stream, logits, M, N, counts);
  return check_launch("diagan_cls_histogram");
}
