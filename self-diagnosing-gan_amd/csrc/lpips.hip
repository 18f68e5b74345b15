// LPIPS for the perceptual path length (include/diagan_lpips.h states the contracts).
//
//   lpips_prep_kernel    a lane per output pixel: reads the three colours of the crop window (NCHW planes or NHWC triples), applies
//                        the scaling layer and stores one float4 with a zero fourth channel.
//   lpips_pool2_kernel   a lane per (output pixel, four channels): the maximum of four float4 in torch's scan order.
//   lpips_sum_parts      a lane per (pixel, four channels): bias + the partial convolutions of the input-channel blocks, added in
//                        float64 in block order, rounded to fp32 once, ReLU.
//   lpips_head_kernel    the distance head of one tap.  A group of L = min(64, C / 4 rounded up to a power of two) lanes owns a
//                        pixel and keeps the pixel's features of BOTH maps in registers (V = 1, 2 or 4 float4 per lane and map), so
//                        each map element is read from memory once: sums of squares -> shuffle butterfly over the group -> the two
//                        reciprocals -> weighted squared differences -> second butterfly.  Everything after the load is float64.  A
//                        workgroup walks HEAD_PIX pixels per group in a fixed order and leaves one partial sum in the workspace.
//   lpips_head_finish    a wave per image adds the image's partials (lane-strided, then the butterfly), divides by the pixel count
//                        and writes or adds the float64 result.
//
// Nothing here depends on B: the run of pixels a workgroup owns, the order inside it and the order of the partials follow from
// (H, W, C) alone.  The butterfly adds a + b in one lane and b + a in its partner, so every lane of a group ends with the same bits.
// Out-of-range pixels and channel vectors are loaded as zeros and go through the same arithmetic (they add exactly 0), which keeps
// every lane of a wave in the shuffles.
//
// This file is compiled with -ffp-contract=off: with f0 r0 - f1 r1 contracted into one fma, identical maps would leave the
// rounding error of one product instead of exactly 0.
#include "common.h"
#include "diagan_lpips.h"

#include <algorithm>

namespace diagan {

constexpr int LP_T = 256;
constexpr int LP_MAX_BLOCKS = 4096;       // prep and pool: memory-bound, cap the grid and stride the rest
constexpr int HEAD_PIX = 16;              // pixels a lane group walks: a workgroup owns HEAD_PIX * (LP_T / L) consecutive pixels
constexpr int HEAD_MAX_C = 1024;

struct LpipsPrep {
  int nhwc, B, H, W, y0, x0, h, w, scale;
};

__global__ __launch_bounds__(LP_T) void lpips_prep_kernel(const float* __restrict__ x, LpipsPrep g, float4* __restrict__ y) {
  const float shift[3] = {-.030f, -.088f, -.188f};
  const float scale[3] = {.458f, .448f, .450f};
  const int64_t plane = (int64_t)g.H * g.W;
  const int64_t items = (int64_t)g.B * g.h * g.w;
  for (int64_t i = (int64_t)blockIdx.x * LP_T + threadIdx.x; i < items; i += (int64_t)gridDim.x * LP_T) {
    const int ox = (int)(i % g.w);
    const int64_t t = i / g.w;
    const int oy = (int)(t % g.h);
    const int64_t b = t / g.h;
    const int64_t pix = (int64_t)(g.y0 + oy) * g.W + (g.x0 + ox);
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c] = g.nhwc ? x[(b * plane + pix) * 3 + c] : x[(b * 3 + c) * plane + pix];
      if (g.scale) v[c] = (v[c] - shift[c]) / scale[c];
    }
    y[i] = make_float4(v[0], v[1], v[2], 0.0f);
  }
}

// torch's max_pool2d scans the window row by row and replaces the running maximum only by a greater value
__device__ __forceinline__ float lp_max4(float a, float b, float c, float d) {
  float m = a;
  if (b > m) m = b;
  if (c > m) m = c;
  if (d > m) m = d;
  return m;
}

__global__ __launch_bounds__(LP_T) void lpips_pool2_kernel(const float4* __restrict__ x, int B, int H, int W, int C4,
                                                           float4* __restrict__ y) {
  const int Ho = H >> 1, Wo = W >> 1;
  const int64_t items = (int64_t)B * Ho * Wo * C4;
  for (int64_t i = (int64_t)blockIdx.x * LP_T + threadIdx.x; i < items; i += (int64_t)gridDim.x * LP_T) {
    const int c = (int)(i % C4);
    int64_t t = i / C4;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const int64_t b = t / Ho;
    const float4* p = x + ((b * H + 2 * oy) * W + 2 * ox) * C4 + c;
    const float4 a = p[0], q = p[C4], r = p[(int64_t)W * C4], s = p[(int64_t)W * C4 + C4];
    y[i] = make_float4(lp_max4(a.x, q.x, r.x, s.x), lp_max4(a.y, q.y, r.y, s.y), lp_max4(a.z, q.z, r.z, s.z),
                       lp_max4(a.w, q.w, r.w, s.w));
  }
}

__global__ __launch_bounds__(LP_T) void lpips_sum_parts_kernel(const float4* __restrict__ parts, int64_t N, int C4, int nparts,
                                                               const float4* __restrict__ bias, int relu, float4* __restrict__ y) {
  const int64_t items = N * C4;
  for (int64_t i = (int64_t)blockIdx.x * LP_T + threadIdx.x; i < items; i += (int64_t)gridDim.x * LP_T) {
    const int c = (int)(i % C4);
    const int64_t n = i / C4;
    const float4 b = bias[c];
    double s[4] = {b.x, b.y, b.z, b.w};
    const float4* p = parts + n * nparts * C4 + c;
    for (int j = 0; j < nparts; ++j) {
      const float4 v = p[(int64_t)j * C4];
      s[0] += v.x, s[1] += v.y, s[2] += v.z, s[3] += v.w;
    }
    float4 o = make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
    if (relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
    y[i] = o;
  }
}

// ---- the head --------------------------------------------------------------------------------------------------------------------
struct HeadPlan {
  int L, V, groups, pix_per_block, chunks;
};

// The ONLY definition of the head's geometry: from (H, W, C), never from B.
static HeadPlan head_plan(int H, int W, int C) {
  HeadPlan p;
  const int c4 = C / 4;
  p.L = 1;
  while (p.L < c4 && p.L < 64) p.L <<= 1;
  p.V = c4 <= 64 ? 1 : (c4 <= 128 ? 2 : 4);
  p.groups = LP_T / p.L;
  p.pix_per_block = p.groups * HEAD_PIX;
  const int64_t P = (int64_t)H * W;
  p.chunks = (int)((P + p.pix_per_block - 1) / p.pix_per_block);
  return p;
}

// sum over the L lanes of a group (L a power of two <= 64, groups aligned to L inside the wave); every lane gets the same bits
__device__ __forceinline__ double group_sum(double v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int V>
__global__ __launch_bounds__(LP_T) void lpips_head_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                          int64_t image_stride, int64_t P, int C4, int L,
                                                          const float4* __restrict__ w, double* __restrict__ part) {
  __shared__ double sh[LP_T];
  const int groups = LP_T / L;
  const int g = threadIdx.x / L, l = threadIdx.x - g * L;
  const int64_t b = blockIdx.y;
  const float4* a0 = reinterpret_cast<const float4*>(f0 + b * image_stride);
  const float4* a1 = reinterpret_cast<const float4*>(f1 + b * image_stride);
  double wd[V][4];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = v * L + l;
    const float4 t = c < C4 ? w[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    wd[v][0] = t.x, wd[v][1] = t.y, wd[v][2] = t.z, wd[v][3] = t.w;
  }
  const int64_t first = (int64_t)blockIdx.x * groups * HEAD_PIX;
  double acc = 0.0;
#pragma unroll 2
  for (int i = 0; i < HEAD_PIX; ++i) {
    const int64_t p = first + (int64_t)i * groups + g;
    const bool in = p < P;
    float4 x0[V], x1[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c = v * L + l;
      const bool ok = in && c < C4;
      x0[v] = ok ? a0[p * C4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
      x1[v] = ok ? a1[p * C4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const double e0[4] = {x0[v].x, x0[v].y, x0[v].z, x0[v].w}, e1[4] = {x1[v].x, x1[v].y, x1[v].z, x1[v].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s0 += e0[k] * e0[k];
        s1 += e1[k] * e1[k];
      }
    }
    s0 = group_sum(s0, L);
    s1 = group_sum(s1, L);
    const double r0 = 1.0 / (sqrt(s0) + 1e-10), r1 = 1.0 / (sqrt(s1) + 1e-10);
    double t = 0.0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const double e0[4] = {x0[v].x, x0[v].y, x0[v].z, x0[v].w}, e1[4] = {x1[v].x, x1[v].y, x1[v].z, x1[v].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double d = e0[k] * r0 - e1[k] * r1;
        t += wd[v][k] * (d * d);
      }
    }
    acc += group_sum(t, L);
  }
  if (l == 0) sh[g] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = sh[0];
    for (int k = 1; k < groups; ++k) s += sh[k];
    part[b * gridDim.x + blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(64) void lpips_head_finish_kernel(const double* __restrict__ part, int chunks, double pixels,
                                                               double* __restrict__ out, int add) {
  const int64_t b = blockIdx.x;
  double s = 0.0;
  for (int j = threadIdx.x; j < chunks; j += 64) s += part[b * chunks + j];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    const double d = s / pixels;
    out[b] = add ? out[b] + d : d;
  }
}

static bool head_shape_ok(int B, int H, int W, int C) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31) && C >= 4 && C <= HEAD_MAX_C && C % 4 == 0;
}

static int lp_blocks(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>(LP_MAX_BLOCKS, (items + LP_T - 1) / LP_T)); }

}  // namespace diagan

using namespace diagan;

DIAGAN_API int diagan_lpips_prep(const float* x, int nhwc, int B, int H, int W, int y0, int x0, int h, int w, int scale, float* y,
                                 void* stream) {
  DG_REQUIRE(x != nullptr && y != nullptr, "diagan_lpips_prep: null pointer");
  DG_REQUIRE(B >= 1 && H >= 1 && W >= 1, "diagan_lpips_prep: bad shape B=%d H=%d W=%d", B, H, W);
  DG_REQUIRE(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && (int64_t)y0 + h <= H && (int64_t)x0 + w <= W,
             "diagan_lpips_prep: window (y0=%d, x0=%d, h=%d, w=%d) outside the %d x %d image", y0, x0, h, w, H, W);
  DG_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 15) == 0, "diagan_lpips_prep: x must be 4-byte and y 16-byte aligned");
  LpipsPrep g = {nhwc != 0, B, H, W, y0, x0, h, w, scale != 0};
  hipLaunchKernelGGL(lpips_prep_kernel, dim3(lp_blocks((int64_t)B * h * w)), dim3(LP_T), 0, (hipStream_t)stream, x, g, (float4*)y);
  return check_launch("diagan_lpips_prep");
}

DIAGAN_API int diagan_lpips_pool2(const float* x, int B, int H, int W, int C, float* y, void* stream) {
  DG_REQUIRE(x != nullptr && y != nullptr, "diagan_lpips_pool2: null pointer");
  DG_REQUIRE(B >= 1 && H >= 2 && W >= 2, "diagan_lpips_pool2: bad shape B=%d H=%d W=%d", B, H, W);
  DG_REQUIRE(C >= 4 && C % 4 == 0, "diagan_lpips_pool2: C=%d is not a positive multiple of 4", C);
  DG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "diagan_lpips_pool2: x and y must be 16-byte aligned");
  const int64_t items = (int64_t)B * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(lpips_pool2_kernel, dim3(lp_blocks(items)), dim3(LP_T), 0, (hipStream_t)stream, (const float4*)x, B, H, W, C / 4,
                     (float4*)y);
  return check_launch("diagan_lpips_pool2");
}

DIAGAN_API int diagan_lpips_sum_parts(const float* parts, int64_t N, int C, int nparts, const float* bias, int relu, float* y,
                                      void* stream) {
  DG_REQUIRE(parts != nullptr && bias != nullptr && y != nullptr, "diagan_lpips_sum_parts: null pointer");
  DG_REQUIRE(N >= 1 && nparts >= 1, "diagan_lpips_sum_parts: N=%ld nparts=%d", (long)N, nparts);
  DG_REQUIRE(C >= 4 && C % 4 == 0, "diagan_lpips_sum_parts: C=%d is not a positive multiple of 4", C);
  DG_REQUIRE((((uintptr_t)parts | (uintptr_t)bias | (uintptr_t)y) & 15) == 0, "diagan_lpips_sum_parts: parts, bias and y must be "
             "16-byte aligned");
  hipLaunchKernelGGL(lpips_sum_parts_kernel, dim3(lp_blocks(N * (C / 4))), dim3(LP_T), 0, (hipStream_t)stream, (const float4*)parts,
                     N, C / 4, nparts, (const float4*)bias, relu != 0, (float4*)y);
  return check_launch("diagan_lpips_sum_parts");
}

DIAGAN_API size_t diagan_lpips_head_ws_bytes(int B, int H, int W, int C) {
  if (!head_shape_ok(B, H, W, C)) return 0;
  return (size_t)B * head_plan(H, W, C).chunks * sizeof(double);
}

DIAGAN_API int diagan_lpips_head(const float* f0, const float* f1, int64_t image_stride, int B, int H, int W, int C, const float* w,
                                 double* out, int add, void* ws, int64_t ws_bytes, void* stream) {
  DG_REQUIRE(f0 != nullptr && f1 != nullptr && w != nullptr && out != nullptr && ws != nullptr, "diagan_lpips_head: null pointer");
  DG_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31),
             "diagan_lpips_head: bad shape B=%d H=%d W=%d (B <= 65535, H W < 2^31)", B, H, W);
  if (!(C >= 4 && C <= HEAD_MAX_C && C % 4 == 0))
    return set_err(DIAGAN_EUNSUP, "diagan_lpips_head: C=%d is not a multiple of 4 in [4, %d]", C, HEAD_MAX_C);
  const int64_t P = (int64_t)H * W;
  DG_REQUIRE(image_stride >= P * C && image_stride % 4 == 0, "diagan_lpips_head: image_stride=%ld for images of %ld elements "
             "(a multiple of 4, at least one image)", (long)image_stride, (long)(P * C));
  DG_REQUIRE((((uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)w) & 15) == 0, "diagan_lpips_head: f0, f1 and w must be 16-byte aligned");
  DG_REQUIRE(((uintptr_t)out & 7) == 0, "diagan_lpips_head: out must be 8-byte aligned");
  const size_t need = diagan_lpips_head_ws_bytes(B, H, W, C);
  DG_REQUIRE(ws_bytes >= (int64_t)need && ((uintptr_t)ws & 7) == 0, "diagan_lpips_head: workspace of %ld bytes, %ld needed "
             "(8-byte aligned)", (long)ws_bytes, (long)need);
  const HeadPlan p = head_plan(H, W, C);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(p.chunks, B);
  double* part = (double*)ws;
  const float4* w4 = (const float4*)w;
  if (p.V == 1)
    hipLaunchKernelGGL(lpips_head_kernel<1>, grid, dim3(LP_T), 0, s, f0, f1, image_stride, P, C / 4, p.L, w4, part);
  else if (p.V == 2)
    hipLaunchKernelGGL(lpips_head_kernel<2>, grid, dim3(LP_T), 0, s, f0, f1, image_stride, P, C / 4, p.L, w4, part);
  else
    hipLaunchKernelGGL(lpips_head_kernel<4>, grid, dim3(LP_T), 0, s, f0, f1, image_stride, P, C / 4, p.L, w4, part);
  int rc = check_launch("diagan_lpips_head");
  if (rc != DIAGAN_OK) return rc;
  hipLaunchKernelGGL(lpips_head_finish_kernel, dim3(B), dim3(64), 0, s, (const double*)part, p.chunks, (double)P, out, add);
  return check_launch("diagan_lpips_head (finish)");
}
