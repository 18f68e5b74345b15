// Non-leaking augmentation (stylegan2/non_leaking.py random_apply_affine + apply_color), DESIGN §8f.
//
// The reference's chain on an NCHW fp32 batch (C = 3):
//   reflect pad (L = pad_low + 6, R = pad_high + 6) -> upfirdn2d(up 2, flipped SYM6 outer product) -> grid_sample over a per-sample
//   affine grid (bilinear, zeros, align_corners=False) -> upfirdn2d(down 2, SYM6 outer product) -> crop -> 4x4 colour matrix.
//
// Forward, two launches:
//   aug_up      X2 = up-FIR of the reflect-padded image, the reflection folded into the index map (the padded image is never
//               written); 6 taps per axis and phase.  X2 [B*3][H2][W2] is the workspace.
//   aug_warp    per 16 x 16 output tile: the 42 x 42 warped 2x samples it needs into LDS (bilinear, sample point computed in
//               float64 from the per-sample affine map), the 12-tap down-FIR along y then x from LDS, the colour matrix.
// Backward (the adjoint of each, G and C constants), three launches, gather form, no float atomics:
//   aug_down_t  gA = down-FIR^T (crop^T (C^T g)) on the 2x grid
//   aug_warp_t  gX2[q] = sum over the 2x output pixels p whose bilinear footprint covers q of w(p, q) gA[p]; the candidates p
//               are the inverse image of q's footprint, and w is recomputed by the forward's own function, so the pairs match
//   aug_up_t    g = up-FIR^T of gX2, summed over the (at most 3 per axis) padded positions that mirror each pixel
// Every sum runs in a fixed order: reruns are bit-identical.
#include "common.h"

namespace diagan {

constexpr int AUG_NP = 18;   // float64 per sample: X0 Xj Xi Y0 Yj Yi, C[3][3], C[:3][3]
constexpr int AUG_K = 12;    // SYM6 taps
constexpr int AUG_PADK = 6;

__constant__ float c_sym6[AUG_K] = {0.015404109327027373f, 0.0034907120842174702f, -0.11799011114819057f, -0.048311742585633f,
                                    0.4910559419267466f,   0.787641141030194f,     0.3379294217276218f,   -0.07263752278646252f,
                                    -0.021060292512300564f, 0.04472490177066578f,  0.0017677118642428036f, -0.007800708325034148f};

struct AugGeom {
  int B, H, W;
  int px1, py1;     // geometric padding, low side (the crop offset)
  int Lx, Ly;       // reflect pad, low side (px1 + 6, py1 + 6)
  int Hp, Wp;       // padded image
  int H2, W2;       // 2x image = warp output grid
};

static int make_geom(int B, int H, int W, int px1, int px2, int py1, int py2, AugGeom* g) {
  DG_REQUIRE(B > 0 && H > 0 && W > 0, "augment: bad shape B=%d H=%d W=%d", B, H, W);
  DG_REQUIRE(px1 >= 0 && px2 >= 0 && py1 >= 0 && py2 >= 0, "augment: negative padding");
  DG_REQUIRE(px1 + AUG_PADK < W && px2 + AUG_PADK < W && py1 + AUG_PADK < H && py2 + AUG_PADK < H,
             "augment: reflect padding (%d, %d, %d, %d) + %d must be smaller than the image (%d x %d)", px1, px2, py1, py2, AUG_PADK,
             H, W);
  g->B = B, g->H = H, g->W = W, g->px1 = px1, g->py1 = py1;
  g->Lx = px1 + AUG_PADK, g->Ly = py1 + AUG_PADK;
  g->Hp = H + py1 + py2 + 2 * AUG_PADK, g->Wp = W + px1 + px2 + 2 * AUG_PADK;
  g->H2 = 2 * g->Hp - AUG_K + 1, g->W2 = 2 * g->Wp - AUG_K + 1;
  DG_REQUIRE((int64_t)B * 3 * g->H2 * g->W2 < ((int64_t)1 << 40), "augment: too large");
  return DIAGAN_OK;
}

__device__ __forceinline__ int reflect(int j, int L, int n) {
  int x = j - L;
  x = x < 0 ? -x : x;
  return x >= n ? 2 * (n - 1) - x : x;
}

// bilinear footprint of the warp at 2x output pixel (row r, col c): top-left tap (x0, y0) and fractions.  The ONE definition both
// directions use.
__device__ __forceinline__ void warp_point(const double* __restrict__ P, int r, int c, int& x0, int& y0, float& fx, float& fy) {
  double ix = fma(P[1], (double)c, fma(P[2], (double)r, P[0]));
  double iy = fma(P[4], (double)c, fma(P[5], (double)r, P[3]));
  ix = fmin(fmax(ix, -4.0e8), 4.0e8);
  iy = fmin(fmax(iy, -4.0e8), 4.0e8);
  const double fx0 = floor(ix), fy0 = floor(iy);
  x0 = (int)fx0, y0 = (int)fy0;
  fx = (float)(ix - fx0), fy = (float)(iy - fy0);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// X2[o] = sum_t s[t] xpad[(o + t) / 2] over (o + t) even: tap t = (o & 1) + 2a reads xpad[ceil(o / 2) + a], a = 0..5
__global__ __launch_bounds__(256) void aug_up(const float* __restrict__ img, float* __restrict__ X2, AugGeom g) {
  const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (ox >= g.W2 || oy >= g.H2) return;
  const float* src = img + (int64_t)blockIdx.z * g.H * g.W;
  int cx[6];
  const int jx = (ox + 1) >> 1, jy = (oy + 1) >> 1, tx0 = ox & 1, ty0 = oy & 1;
#pragma unroll
  for (int a = 0; a < 6; ++a) cx[a] = reflect(jx + a, g.Lx, g.W);
  float acc = 0.f;
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const float* row = src + (int64_t)reflect(jy + b, g.Ly, g.H) * g.W;
    float h = 0.f;
#pragma unroll
    for (int a = 0; a < 6; ++a) h = fmaf(c_sym6[tx0 + 2 * a], row[cx[a]], h);
    acc = fmaf(c_sym6[ty0 + 2 * b], h, acc);
  }
  X2[((int64_t)blockIdx.z * g.H2 + oy) * g.W2 + ox] = acc;
}

constexpr int WT = 16;                    // output tile
constexpr int WA = 2 * WT + AUG_K - 2;    // 42: 2x samples per tile side
constexpr int WLD = WA + 1;

__global__ __launch_bounds__(256) void aug_warp(const float* __restrict__ X2, const double* __restrict__ params,
                                                float* __restrict__ out, AugGeom g) {
  __shared__ float As[3][WA][WLD];
  __shared__ float Vs[3][WT][WLD];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int oy0 = blockIdx.y * WT, ox0 = blockIdx.x * WT;
  const int ay0 = 2 * (oy0 + g.py1), ax0 = 2 * (ox0 + g.px1);   // 2x-grid origin of the tile's footprint
  const double* P = params + (int64_t)b * AUG_NP;
  const int64_t plane = (int64_t)g.H2 * g.W2;
  const float* X = X2 + (int64_t)b * 3 * plane;
  for (int idx = tid; idx < WA * WA; idx += 256) {
    const int r = idx / WA, c = idx - r * WA, pr = ay0 + r, pc = ax0 + c;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if (pr < g.H2 && pc < g.W2) {
      int x0, y0;
      float fx, fy;
      warp_point(P, pr, pc, x0, y0, fx, fy);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const int y = y0 + dy;
        if (y < 0 || y >= g.H2) continue;
        const float wy = dy ? fy : 1.f - fy;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int x = x0 + dx;
          if (x < 0 || x >= g.W2) continue;
          const float w = (dx ? fx : 1.f - fx) * wy;
          const int64_t o = (int64_t)y * g.W2 + x;
          v0 = fmaf(w, X[o], v0), v1 = fmaf(w, X[plane + o], v1), v2 = fmaf(w, X[2 * plane + o], v2);
        }
      }
    }
    As[0][r][c] = v0, As[1][r][c] = v1, As[2][r][c] = v2;
  }
  __syncthreads();
  // y[o] = sum_t s[11 - t] a[2 o + t]
  for (int idx = tid; idx < 3 * WT * WA; idx += 256) {
    const int ch = idx / (WT * WA), rem = idx - ch * WT * WA, r = rem / WA, c = rem - r * WA;
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < AUG_K; ++t) acc = fmaf(c_sym6[AUG_K - 1 - t], As[ch][2 * r + t][c], acc);
    Vs[ch][r][c] = acc;
  }
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15, oy = oy0 + ty, ox = ox0 + tx;
  if (oy >= g.H || ox >= g.W) return;
  float v[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < AUG_K; ++t) acc = fmaf(c_sym6[AUG_K - 1 - t], Vs[ch][ty][2 * tx + t], acc);
    v[ch] = acc;
  }
  const int64_t hw = (int64_t)g.H * g.W, o = (int64_t)b * 3 * hw + (int64_t)oy * g.W + ox;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double* m = P + 6 + 3 * k;
    out[o + k * hw] = fmaf((float)m[2], v[2], fmaf((float)m[1], v[1], fmaf((float)m[0], v[0], (float)P[15 + k])));
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// gA[Y][X] = sum over taps ty, tx with Y - ty, X - tx even of s[11 - ty] s[11 - tx] gd[(Y - ty) / 2 - py1][(X - tx) / 2 - px1],
// gd = C^T g (applied once after the taps: the map is linear)
__global__ __launch_bounds__(256) void aug_down_t(const float* __restrict__ gout, const double* __restrict__ params,
                                                  float* __restrict__ gA, AugGeom g) {
  const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (X >= g.W2 || Y >= g.H2) return;
  const int64_t hw = (int64_t)g.H * g.W;
  const float* go = gout + (int64_t)b * 3 * hw;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int ty = Y & 1; ty < AUG_K; ty += 2) {
    const int y = (Y - ty) / 2 - g.py1;
    if (Y < ty || y < 0 || y >= g.H) continue;
    float h0 = 0.f, h1 = 0.f, h2 = 0.f;
    for (int tx = X & 1; tx < AUG_K; tx += 2) {
      const int x = (X - tx) / 2 - g.px1;
      if (X < tx || x < 0 || x >= g.W) continue;
      const float w = c_sym6[AUG_K - 1 - tx];
      const int64_t o = (int64_t)y * g.W + x;
      h0 = fmaf(w, go[o], h0), h1 = fmaf(w, go[hw + o], h1), h2 = fmaf(w, go[2 * hw + o], h2);
    }
    const float w = c_sym6[AUG_K - 1 - ty];
    s0 = fmaf(w, h0, s0), s1 = fmaf(w, h1, s1), s2 = fmaf(w, h2, s2);
  }
  const double* m = params + (int64_t)b * AUG_NP + 6;   // out_k = sum_c m[k][c] in_c  ->  gin_c = sum_k m[k][c] g_k
  const int64_t plane = (int64_t)g.H2 * g.W2, o = (int64_t)b * 3 * plane + (int64_t)Y * g.W2 + X;
#pragma unroll
  for (int c = 0; c < 3; ++c) gA[o + c * plane] = fmaf((float)m[6 + c], s2, fmaf((float)m[3 + c], s1, (float)m[c] * s0));
}

// gX2[q] = sum_p w(p, q) gA[p].  p -> (ix, iy) is affine with linear part L = [[Xj, Xi], [Yj, Yi]] (p = (col, row)); q's weight is
// non-zero only for |ix - qx| < 1, |iy - qy| < 1, whose preimage lies in the box centre L^-1 (q - o) +- (|L^-1| 1); the box is
// widened by one pixel and every candidate is decided by warp_point itself.  gA is zero outside the down-FIR's footprint
// (rows 2 py1 .. 2 (py1 + H) + 9), so candidates are clipped to it.
__global__ __launch_bounds__(256) void aug_warp_t(const float* __restrict__ gA, const double* __restrict__ params,
                                                  float* __restrict__ gX2, AugGeom g) {
  const int qx = blockIdx.x * 64 + (threadIdx.x & 63), qy = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (qx >= g.W2 || qy >= g.H2) return;
  const double* P = params + (int64_t)b * AUG_NP;
  const double det = P[1] * P[5] - P[2] * P[4];
  const double i00 = P[5] / det, i01 = -P[2] / det, i10 = -P[4] / det, i11 = P[1] / det;
  const double dx = qx - P[0], dy = qy - P[3];
  const double cc = i00 * dx + i01 * dy, cr = i10 * dx + i11 * dy;
  const double hc = fabs(i00) + fabs(i01), hr = fabs(i10) + fabs(i11);
  const int rlo = 2 * g.py1, rhi = min(g.H2 - 1, 2 * (g.py1 + g.H) + AUG_K - 3);
  const int clo = 2 * g.px1, chi = min(g.W2 - 1, 2 * (g.px1 + g.W) + AUG_K - 3);
  const int r0 = (int)fmax((double)rlo, floor(cr - hr) - 1), r1 = (int)fmin((double)rhi, ceil(cr + hr) + 1);
  const int c0 = (int)fmax((double)clo, floor(cc - hc) - 1), c1 = (int)fmin((double)chi, ceil(cc + hc) + 1);
  const int64_t plane = (int64_t)g.H2 * g.W2;
  const float* G = gA + (int64_t)b * 3 * plane;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int r = r0; r <= r1; ++r) {
    for (int c = c0; c <= c1; ++c) {
      int x0, y0;
      float fx, fy;
      warp_point(P, r, c, x0, y0, fx, fy);
      const int ddx = qx - x0, ddy = qy - y0;
      if ((unsigned)ddx > 1u || (unsigned)ddy > 1u) continue;
      const float w = (ddx ? fx : 1.f - fx) * (ddy ? fy : 1.f - fy);
      const int64_t o = (int64_t)r * g.W2 + c;
      a0 = fmaf(w, G[o], a0), a1 = fmaf(w, G[plane + o], a1), a2 = fmaf(w, G[2 * plane + o], a2);
    }
  }
  const int64_t o = (int64_t)b * 3 * plane + (int64_t)qy * g.W2 + qx;
  gX2[o] = a0, gX2[o + plane] = a1, gX2[o + 2 * plane] = a2;
}

// padded positions j with reflect(j) == x, ascending
__device__ __forceinline__ int mirrors(int x, int L, int n, int np, int* j) {
  int k = 0;
  if (x >= 1 && x <= L) j[k++] = L - x;                   // left reflection
  j[k++] = L + x;
  const int jr = L + 2 * (n - 1) - x;                     // right reflection
  if (x <= n - 2 && jr < np) j[k++] = jr;
  return k;
}

// g[y][x] = sum over mirror positions (jy, jx) of sum_{ty, tx} s[ty] s[tx] gX2[2 jy - ty][2 jx - tx]
__global__ __launch_bounds__(256) void aug_up_t(const float* __restrict__ gX2, float* __restrict__ gimg, AugGeom g) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= g.W || y >= g.H) return;
  const float* src = gX2 + (int64_t)blockIdx.z * g.H2 * g.W2;
  int jx[3], jy[3];
  const int nx = mirrors(x, g.Lx, g.W, g.Wp, jx), ny = mirrors(y, g.Ly, g.H, g.Hp, jy);
  float acc = 0.f;
  for (int a = 0; a < ny; ++a) {
    for (int ty = 0; ty < AUG_K; ++ty) {
      const int Y = 2 * jy[a] - ty;
      if (Y < 0 || Y >= g.H2) continue;
      const float* row = src + (int64_t)Y * g.W2;
      float h = 0.f;
      for (int b = 0; b < nx; ++b) {
#pragma unroll
        for (int tx = 0; tx < AUG_K; ++tx) {
          const int X = 2 * jx[b] - tx;
          if (X >= 0 && X < g.W2) h = fmaf(c_sym6[tx], row[X], h);
        }
      }
      acc = fmaf(c_sym6[ty], h, acc);
    }
  }
  gimg[((int64_t)blockIdx.z * g.H + y) * g.W + x] = acc;
}

}  // namespace diagan

using namespace diagan;

DIAGAN_API int diagan_augment_params(void) { return AUG_NP; }

DIAGAN_API int diagan_augment_workspace(int B, int H, int W, int px1, int px2, int py1, int py2, int backward, int64_t* bytes) {
  AugGeom g;
  int rc = make_geom(B, H, W, px1, px2, py1, py2, &g);
  if (rc) return rc;
  DG_REQUIRE(bytes, "augment_workspace: bytes is NULL");
  *bytes = (backward ? 2 : 1) * (int64_t)B * 3 * g.H2 * g.W2 * (int64_t)sizeof(float);
  return DIAGAN_OK;
}

DIAGAN_API int diagan_augment_forward(const float* img, const double* params, int B, int H, int W, int px1, int px2, int py1, int py2,
                                      float* out, void* workspace, void* stream) {
  AugGeom g;
  int rc = make_geom(B, H, W, px1, px2, py1, py2, &g);
  if (rc) return rc;
  DG_REQUIRE(img && params && out && workspace, "augment_forward: NULL pointer");
  DG_REQUIRE(out != img, "augment_forward: out must not alias img");
  hipStream_t s = (hipStream_t)stream;
  float* X2 = (float*)workspace;
  aug_up<<<dim3(cdiv(g.W2, 64), cdiv(g.H2, 4), B * 3), 256, 0, s>>>(img, X2, g);
  aug_warp<<<dim3(cdiv(W, WT), cdiv(H, WT), B), 256, 0, s>>>(X2, params, out, g);
  return check_launch("augment_forward");
}

DIAGAN_API int diagan_augment_backward(const float* gout, const double* params, int B, int H, int W, int px1, int px2, int py1,
                                       int py2, float* gimg, void* workspace, void* stream) {
  AugGeom g;
  int rc = make_geom(B, H, W, px1, px2, py1, py2, &g);
  if (rc) return rc;
  DG_REQUIRE(gout && params && gimg && workspace, "augment_backward: NULL pointer");
  DG_REQUIRE(gimg != gout, "augment_backward: gimg must not alias gout");
  hipStream_t s = (hipStream_t)stream;
  float* gA = (float*)workspace;
  float* gX2 = gA + (int64_t)B * 3 * g.H2 * g.W2;
  const dim3 grid2(cdiv(g.W2, 64), cdiv(g.H2, 4), B);
  aug_down_t<<<grid2, 256, 0, s>>>(gout, params, gA, g);
  aug_warp_t<<<grid2, 256, 0, s>>>(gA, params, gX2, g);
  aug_up_t<<<dim3(cdiv(W, 64), cdiv(H, 4), B * 3), 256, 0, s>>>(gX2, gimg, g);
  return check_launch("augment_backward");
}
