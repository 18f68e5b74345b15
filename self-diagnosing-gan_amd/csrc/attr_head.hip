// The head of the CelebA attribute classifier (the diagan_attr_* part of include/diagan_lpips.h states the contracts).
//
//   attr_pool_flatten_kernel   a lane per output element: the mean over its adaptive bin, written in torchvision's flatten order.
//   attr_dense_fwd_kernel      Y = act(X W^T + b) keep on v_mfma_f32_16x16x4_f32.  A workgroup owns EVERY row (MT tiles of 16, at
//                              most 128 rows) and 16 columns; wave v of eight takes the K steps v, v + 8, ... of 32, so each element of X and
//                              W is loaded by exactly one lane of the workgroup, straight into MFMA operands (a lane reads 8
//                              consecutive k of its row: the k order inside a step is permuted the same way for both operands).
//                              The next step's operands are loaded before the current step's products.  Waves 1..7 leave their
//                              tiles in LDS, wave 0 adds them in wave order and applies bias, ReLU and the keep-mask.
//   attr_dense_small_kernel    N <= 4: a wave per row, N dot products at once, the shuffle butterfly.
//   attr_dense_dgrad_kernel    dX = dZ W with dZ = dY [Y > 0] keep formed at the load.  A workgroup owns every row and 32 columns
//                              of K (two tiles, 128 bytes of each W row); the waves split N in steps of 16, dY, Y and the mask come in
//                              16-byte loads where N allows, the next step's operands are in flight during the products.
//   attr_dense_wgrad_kernel    g = dZ^T X and the SGD step.  The reduction is the batch (<= 128), so a wave keeps its 16 columns
//                              of dZ in 32 registers for the whole launch and walks a run of K, 32 columns a step: 2 x 32 products
//                              into two tiles, then buf = mu buf + g, w -= lr buf on the accumulator's own elements.
//   attr_ce_kernel             a lane per row in float64; one workgroup; thread 0 adds to the accumulators.
//   attr_count_kernel          likewise.
//
// Out-of-range rows, columns and reduction indices are loaded as zeros from no address at all (the select is on the pointer
// arithmetic's guard, not on a clamped address) and go through the same arithmetic; stores are guarded.
#include "common.h"
#include "diagan_lpips.h"

#include <algorithm>

namespace diagan {

using at4 = __attribute__((ext_vector_type(4))) float;

constexpr int AT_T = 256;
constexpr int FW_WAVES = 8;            // waves of a dense-forward workgroup: two per SIMD, one's loads under the other's products
constexpr int AT_MAX_BLOCKS = 4096;
constexpr int AT_ROWS = 128;          // rows a dense workgroup keeps resident
constexpr int AT_SMALL_N = 4;         // widest layer of the small path
constexpr int WG_KSPAN = 256;         // columns of K a weight-gradient workgroup walks
constexpr int AT_MAX_CLASSES = 64;

__device__ __forceinline__ at4 mfma16(float a, float b, at4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ---- pool + flatten ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AT_T) void attr_pool_flatten_kernel(const float* __restrict__ x, int B, int H, int W, int C,
                                                                 float* __restrict__ y) {
  const int64_t items = (int64_t)B * C * 49;
  for (int64_t i = (int64_t)blockIdx.x * AT_T + threadIdx.x; i < items; i += (int64_t)gridDim.x * AT_T) {
    const int j = (int)(i % 7);
    int64_t t = i / 7;
    const int bi = (int)(t % 7);
    t /= 7;
    const int c = (int)(t % C);
    const int64_t b = t / C;
    const int r0 = (int)(((int64_t)bi * H) / 7), r1 = (int)((((int64_t)bi + 1) * H + 6) / 7);
    const int c0 = (int)(((int64_t)j * W) / 7), c1 = (int)((((int64_t)j + 1) * W + 6) / 7);
    float s = 0.f;
    for (int r = r0; r < r1; ++r)
      for (int q = c0; q < c1; ++q) s += x[((b * H + r) * W + q) * C + c];
    y[i] = s / (float)((int64_t)(r1 - r0) * (c1 - c0));
  }
}

// ---- dZ at the load ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dz_of(float dy, float y, float keep, bool has_y) { return (has_y && !(y > 0.f)) ? 0.f : dy * keep; }

__device__ __forceinline__ float dz_at(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ mask,
                                       float drop_scale, int64_t i) {
  const float keep = mask ? mask[i] * drop_scale : 1.f;
  return dz_of(dy[i], y ? y[i] : 1.f, keep, y != nullptr);
}

// 8 consecutive values p[k .. k + 8) of a row of length K, zeros past the end; two 16-byte loads when `vec` and wholly inside
__device__ __forceinline__ void load8(const float* __restrict__ p, bool row_ok, int k, int K, bool vec, float (&v)[8]) {
  if (row_ok && vec && k + 8 <= K) {
    const at4 a = *reinterpret_cast<const at4*>(p + k), b = *reinterpret_cast<const at4*>(p + k + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = a[e], v[4 + e] = b[e];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (row_ok && k + e < K) ? p[k + e] : 0.f;
  }
}

// ---- dense forward ----------------------------------------------------------------------------------------------------------------
template <int MT>
__global__ __launch_bounds__(FW_WAVES * 64) void attr_dense_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, int M, int K, int N, int relu,
                                                              const float* __restrict__ mask, float drop_scale,
                                                              float* __restrict__ y, int vec) {
  __shared__ float red[FW_WAVES - 1][MT * 16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.y * AT_ROWS, n0 = blockIdx.x * 16;
  const bool n_ok = n0 + li < N;
  const float* wrow = w + (int64_t)(n_ok ? n0 + li : 0) * K;
  const float* xrow[MT];
  bool m_ok[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    m_ok[t] = m0 + t * 16 + li < M;
    xrow[t] = x + (int64_t)(m_ok[t] ? m0 + t * 16 + li : 0) * K;
  }
  at4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = at4{0.f, 0.f, 0.f, 0.f};
  const int steps = (K + 31) / 32;
  float a[MT][8], b[8];
  if (wave < steps) {
    load8(wrow, n_ok, wave * 32 + g * 8, K, vec, b);
#pragma unroll
    for (int t = 0; t < MT; ++t) load8(xrow[t], m_ok[t], wave * 32 + g * 8, K, vec, a[t]);
  }
  for (int s = wave; s < steps; s += FW_WAVES) {
    float an[MT][8], bn[8];
    const bool more = s + FW_WAVES < steps;
    if (more) {
      const int kb = (s + FW_WAVES) * 32 + g * 8;
      load8(wrow, n_ok, kb, K, vec, bn);
#pragma unroll
      for (int t = 0; t < MT; ++t) load8(xrow[t], m_ok[t], kb, K, vec, an[t]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = mfma16(a[t][e], b[e], acc[t]);
    if (more) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        b[e] = bn[e];
#pragma unroll
        for (int t = 0; t < MT; ++t) a[t][e] = an[t][e];
      }
    }
  }
  // C/D map of 16x16x4: column = lane & 15, row = (lane >> 4) * 4 + register
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave - 1][t * 16 + g * 4 + r][li] = acc[t][r];
  }
  __syncthreads();
  if (wave == 0) {
    const int n = n0 + li;
    const float bv = (bias && n_ok) ? bias[n] : 0.f;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = t * 16 + g * 4 + r, m = m0 + row;
        float v = acc[t][r];
#pragma unroll
        for (int q = 0; q < FW_WAVES - 1; ++q) v += red[q][row][li];
        v += bv;
        if (relu) v = fmaxf(v, 0.f);
        if (m < M && n_ok) {
          const int64_t o = (int64_t)m * N + n;
          if (mask) v *= mask[o] * drop_scale;
          y[o] = v;
        }
      }
  }
}

__global__ __launch_bounds__(AT_T) void attr_dense_small_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, int M, int K, int N, int relu,
                                                                const float* __restrict__ mask, float drop_scale,
                                                                float* __restrict__ y, int vec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * 4 + wave;
  if (m >= M) return;                  // a whole wave leaves; nothing below synchronises the workgroup
  const float* xr = x + (int64_t)m * K;
  float acc[AT_SMALL_N] = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    for (int k = lane * 4; k < K; k += 256) {
      const at4 xv = *reinterpret_cast<const at4*>(xr + k);
#pragma unroll
      for (int n = 0; n < AT_SMALL_N; ++n)
        if (n < N) {
          const at4 wv = *reinterpret_cast<const at4*>(w + (int64_t)n * K + k);
          acc[n] += xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
        }
    }
  } else {
    for (int k = lane; k < K; k += 64) {
      const float xv = xr[k];
#pragma unroll
      for (int n = 0; n < AT_SMALL_N; ++n)
        if (n < N) acc[n] += xv * w[(int64_t)n * K + k];
    }
  }
#pragma unroll
  for (int n = 0; n < AT_SMALL_N; ++n) {
    const float s = wave_sum(acc[n]);
    if (lane == n && n < N) {
      float v = s + (bias ? bias[n] : 0.f);
      if (relu) v = fmaxf(v, 0.f);
      const int64_t o = (int64_t)m * N + n;
      if (mask) v *= mask[o] * drop_scale;
      y[o] = v;
    }
  }
}

// ---- data gradient ----------------------------------------------------------------------------------------------------------------
// the operands of one reduction step of the data gradient: a[t][e] = dZ[row tile t][nb + e], b[e][c] = W[nb + e][k0 + 16 c + li]
template <int MT>
__device__ __forceinline__ void dgrad_load(const float* __restrict__ dy, const float* __restrict__ yv, const float* __restrict__ mask,
                                           float drop_scale, const float* __restrict__ w, int M, int K, int N, int m0, int k0,
                                           int li, int nb, bool vec, float (&a)[MT][4], float (&b)[4][2]) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int n = nb + e, k = k0 + c * 16 + li;
      b[e][c] = (n < N && k < K) ? w[(int64_t)n * K + k] : 0.f;
    }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = m0 + t * 16 + li;
    const int64_t o = (int64_t)m * N + nb;
    if (m < M && vec && nb + 4 <= N) {
      const at4 d = *reinterpret_cast<const at4*>(dy + o);
      const at4 one = at4{1.f, 1.f, 1.f, 1.f};
      const at4 yy = yv ? *reinterpret_cast<const at4*>(yv + o) : one;
      const at4 mk = mask ? *reinterpret_cast<const at4*>(mask + o) : one;
#pragma unroll
      for (int e = 0; e < 4; ++e) a[t][e] = dz_of(d[e], yy[e], mask ? mk[e] * drop_scale : 1.f, yv != nullptr);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) a[t][e] = (m < M && nb + e < N) ? dz_at(dy, yv, mask, drop_scale, o + e) : 0.f;
    }
  }
}

template <int MT>
__global__ __launch_bounds__(AT_T) void attr_dense_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ yv,
                                                                const float* __restrict__ mask, float drop_scale,
                                                                const float* __restrict__ w, int M, int K, int N,
                                                                float* __restrict__ dx, int vec) {
  __shared__ float red[3][MT * 16][33];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.y * AT_ROWS, k0 = blockIdx.x * 32;
  at4 acc[MT][2];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t][0] = acc[t][1] = at4{0.f, 0.f, 0.f, 0.f};
  const int steps = (N + 15) / 16;
  float a[MT][4], b[4][2];
  if (wave < steps) dgrad_load<MT>(dy, yv, mask, drop_scale, w, M, K, N, m0, k0, li, wave * 16 + g * 4, vec, a, b);
  for (int s = wave; s < steps; s += 4) {
    float an[MT][4], bn[4][2];
    const bool more = s + 4 < steps;
    if (more) dgrad_load<MT>(dy, yv, mask, drop_scale, w, M, K, N, m0, k0, li, (s + 4) * 16 + g * 4, vec, an, bn);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t][c] = mfma16(a[t][e], b[e][c], acc[t][c]);
    if (more) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        b[e][0] = bn[e][0], b[e][1] = bn[e][1];
#pragma unroll
        for (int t = 0; t < MT; ++t) a[t][e] = an[t][e];
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave - 1][t * 16 + g * 4 + r][c * 16 + li] = acc[t][c][r];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = t * 16 + g * 4 + r, col = c * 16 + li;
          const int m = m0 + row, k = k0 + col;
          const float v = ((acc[t][c][r] + red[0][row][col]) + red[1][row][col]) + red[2][row][col];
          if (m < M && k < K) dx[(int64_t)m * K + k] = v;
        }
  }
}

// ---- weight gradient + SGD ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AT_T) void attr_dense_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ yv,
                                                                const float* __restrict__ mask, float drop_scale,
                                                                const float* __restrict__ x, int M, int K, int N, float lr,
                                                                float mu, float* __restrict__ w, float* __restrict__ bias,
                                                                float* __restrict__ buf_w, float* __restrict__ buf_b,
                                                                float* __restrict__ g_w, float* __restrict__ g_b) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int nt = blockIdx.y * 64 + wave * 16;         // this wave's 16 rows of W
  const int na = nt + li;                             // A operand: A[i = column n of dZ][reduction m]
  float a[32];                                        // a[s] = dZ[m = 4 s + g][na]
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    const int m = s * 4 + g;
    a[s] = (m < M && na < N) ? dz_at(dy, yv, mask, drop_scale, (int64_t)m * N + na) : 0.f;
  }
  if (blockIdx.x == 0 && (g_w ? g_b != nullptr : bias != nullptr)) {
    float sb = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) sb += a[s];
    sb += __shfl_xor(sb, 16, 64);
    sb += __shfl_xor(sb, 32, 64);
    if (g == 0 && na < N) {
      if (g_w) {
        g_b[na] = sb;
      } else {
        const float bb = mu * buf_b[na] + sb;
        buf_b[na] = bb;
        bias[na] -= lr * bb;
      }
    }
  }
  const int ms = (M + 3) / 4;
  const int kend = (int)min((int64_t)K, ((int64_t)blockIdx.x + 1) * WG_KSPAN);
  for (int kc = blockIdx.x * WG_KSPAN; kc < kend; kc += 32) {
    at4 acc[2] = {at4{0.f, 0.f, 0.f, 0.f}, at4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int sc = 0; sc < 4; ++sc) {
      if (sc * 8 < ms) {                              // uniform: eight reduction steps (32 rows of the batch) at a time
        float b[8][2];
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int m = (sc * 8 + q) * 4 + g, k = kc + c * 16 + li;
            b[q][c] = (m < M && k < K) ? x[(int64_t)m * K + k] : 0.f;
          }
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[c] = mfma16(a[sc * 8 + q], b[q][c], acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = nt + g * 4 + r, k = kc + c * 16 + li;
        if (n < N && k < K) {
          const int64_t o = (int64_t)n * K + k;
          const float gv = acc[c][r];
          if (g_w) {
            g_w[o] = gv;
          } else {
            const float bb = mu * buf_w[o] + gv;
            buf_w[o] = bb;
            w[o] -= lr * bb;
          }
        }
      }
  }
}

// ---- cross-entropy and count ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long wave_sum_long(long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(AT_T) void attr_ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int M,
                                                       int N, float* __restrict__ dlogit, double* __restrict__ loss_acc,
                                                       int64_t* __restrict__ correct_acc) {
  __shared__ double sh_l[AT_T / 64];
  __shared__ long sh_c[AT_T / 64];
  double lsum = 0.0;
  long corr = 0;
  for (int m = threadIdx.x; m < M; m += AT_T) {
    const float* z = logits + (int64_t)m * N;
    float zmax = z[0];
    int arg = 0;
    for (int n = 1; n < N; ++n)
      if (z[n] > zmax) zmax = z[n], arg = n;         // only a greater value replaces the maximum: the first one wins
    const double mx = (double)zmax;
    double se = 0.0;
    for (int n = 0; n < N; ++n) se += exp((double)z[n] - mx);
    const int64_t t = target[m];
    const bool t_ok = t >= 0 && t < N;               // a target outside [0, N) is a caller's error; it reads nothing out of range
    lsum += log(se) - ((t_ok ? (double)z[t] : mx) - mx);
    corr += (t_ok && arg == (int)t) ? 1 : 0;
    for (int n = 0; n < N; ++n) {
      const double p = exp((double)z[n] - mx) / se;
      dlogit[(int64_t)m * N + n] = (float)((p - (n == t ? 1.0 : 0.0)) / (double)M);
    }
  }
  lsum = wave_sum(lsum);
  corr = wave_sum_long(corr);
  if ((threadIdx.x & 63) == 0) sh_l[threadIdx.x >> 6] = lsum, sh_c[threadIdx.x >> 6] = corr;
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = sh_l[0];
    long c = sh_c[0];
    for (int v = 1; v < AT_T / 64; ++v) l += sh_l[v], c += sh_c[v];
    loss_acc[0] += l / (double)M;
    correct_acc[0] += c;
  }
}

__global__ __launch_bounds__(AT_T) void attr_count_kernel(const float* __restrict__ logits, int M, int N,
                                                          int64_t* __restrict__ counter) {
  __shared__ long sh_c[AT_T / 64];
  long cnt = 0;
  for (int m = threadIdx.x; m < M; m += AT_T) {
    const float* z = logits + (int64_t)m * N;
    bool pos = false;
    for (int n = 1; n < N; ++n) pos = pos || z[n] > z[0];     // the first maximum is past column 0 iff some later value is greater
    cnt += pos ? 1 : 0;
  }
  cnt = wave_sum_long(cnt);
  if ((threadIdx.x & 63) == 0) sh_c[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    long c = sh_c[0];
    for (int v = 1; v < AT_T / 64; ++v) c += sh_c[v];
    counter[0] += c;
  }
}

static int at_blocks(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>(AT_MAX_BLOCKS, (items + AT_T - 1) / AT_T)); }

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int row_tiles(int M) {                         // 16-row tiles a workgroup holds: 1, 2, 4 or 8
  const int t = (std::min(M, AT_ROWS) + 15) / 16;
  return t <= 1 ? 1 : (t <= 2 ? 2 : (t <= 4 ? 4 : 8));
}

}  // namespace diagan

using namespace diagan;

DIAGAN_API int diagan_attr_pool_flatten(const float* x, int B, int H, int W, int C, float* y, void* stream) {
  DG_REQUIRE(x != nullptr && y != nullptr, "diagan_attr_pool_flatten: null pointer");
  DG_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= (1 << 20) && W <= (1 << 20),
             "diagan_attr_pool_flatten: bad shape B=%d H=%d W=%d C=%d (H, W in [1, 2^20])", B, H, W, C);
  hipLaunchKernelGGL(attr_pool_flatten_kernel, dim3(at_blocks((int64_t)B * C * 49)), dim3(AT_T), 0, (hipStream_t)stream, x, B, H, W,
                     C, y);
  return check_launch("diagan_attr_pool_flatten");
}

DIAGAN_API int diagan_attr_dense_fwd(const float* x, const float* w, const float* bias, int M, int K, int N, int relu,
                                     const float* mask, float drop_scale, float* y, void* stream) {
  DG_REQUIRE(x != nullptr && w != nullptr && y != nullptr, "diagan_attr_dense_fwd: null pointer");
  DG_REQUIRE(M >= 1 && K >= 1 && K <= (1 << 30) && N >= 1, "diagan_attr_dense_fwd: bad shape M=%d K=%d N=%d", M, K, N);
  DG_REQUIRE((M + AT_ROWS - 1) / AT_ROWS <= 65535, "diagan_attr_dense_fwd: M=%d is more than 65535 blocks of %d rows", M, AT_ROWS);
  const int vec = K % 4 == 0 && aligned16(x) && aligned16(w);
  hipStream_t s = (hipStream_t)stream;
  if (N <= AT_SMALL_N) {
    hipLaunchKernelGGL(attr_dense_small_kernel, dim3((M + 3) / 4), dim3(AT_T), 0, s, x, w, bias, M, K, N, relu != 0, mask,
                       drop_scale, y, vec);
    return check_launch("diagan_attr_dense_fwd (small)");
  }
  const dim3 grid((N + 15) / 16, (M + AT_ROWS - 1) / AT_ROWS);
  switch (row_tiles(M)) {
#define DG_FWD(MT)                                                                                                              \
  case MT:                                                                                                                      \
    hipLaunchKernelGGL(attr_dense_fwd_kernel<MT>, grid, dim3(FW_WAVES * 64), 0, s, x, w, bias, M, K, N, relu != 0, mask, drop_scale, y, vec); \
    break;
    DG_FWD(1) DG_FWD(2) DG_FWD(4) DG_FWD(8)
#undef DG_FWD
  }
  return check_launch("diagan_attr_dense_fwd");
}

DIAGAN_API int diagan_attr_dense_dgrad(const float* dy, const float* y, const float* mask, float drop_scale, const float* w, int M,
                                       int K, int N, float* dx, void* stream) {
  DG_REQUIRE(dy != nullptr && w != nullptr && dx != nullptr, "diagan_attr_dense_dgrad: null pointer");
  DG_REQUIRE(M >= 1 && K >= 1 && K <= (1 << 30) && N >= 1 && N <= (1 << 30), "diagan_attr_dense_dgrad: bad shape M=%d K=%d N=%d", M, K, N);
  DG_REQUIRE((M + AT_ROWS - 1) / AT_ROWS <= 65535, "diagan_attr_dense_dgrad: M=%d is more than 65535 blocks of %d rows", M, AT_ROWS);
  hipStream_t s = (hipStream_t)stream;
  const int vec = N % 4 == 0 && aligned16(dy) && (y == nullptr || aligned16(y)) && (mask == nullptr || aligned16(mask));
  const dim3 grid((K + 31) / 32, (M + AT_ROWS - 1) / AT_ROWS);
  switch (row_tiles(M)) {
#define DG_DGRAD(MT)                                                                                                        \
  case MT:                                                                                                                  \
    hipLaunchKernelGGL(attr_dense_dgrad_kernel<MT>, grid, dim3(AT_T), 0, s, dy, y, mask, drop_scale, w, M, K, N, dx, vec); \
    break;
    DG_DGRAD(1) DG_DGRAD(2) DG_DGRAD(4) DG_DGRAD(8)
#undef DG_DGRAD
  }
  return check_launch("diagan_attr_dense_dgrad");
}

DIAGAN_API int diagan_attr_dense_wgrad_sgd(const float* dy, const float* y, const float* mask, float drop_scale, const float* x,
                                           int M, int K, int N, float lr, float momentum, float* w, float* bias, float* buf_w,
                                           float* buf_b, float* g_w, float* g_b, void* stream) {
  DG_REQUIRE(dy != nullptr && x != nullptr, "diagan_attr_dense_wgrad_sgd: null pointer");
  DG_REQUIRE(K >= 1 && K <= (1 << 30) && N >= 1 && N <= (1 << 30), "diagan_attr_dense_wgrad_sgd: bad shape K=%d N=%d", K, N);
  if (!(M >= 1 && M <= AT_ROWS))
    return set_err(DIAGAN_EUNSUP, "diagan_attr_dense_wgrad_sgd: a batch of %d rows (1 .. %d: the sum over the batch stays in one wave)",
                   M, AT_ROWS);
  if (g_w == nullptr) {
    DG_REQUIRE(w != nullptr && buf_w != nullptr, "diagan_attr_dense_wgrad_sgd: the step needs w and buf_w");
    DG_REQUIRE((bias == nullptr) == (buf_b == nullptr), "diagan_attr_dense_wgrad_sgd: bias and buf_b go together");
  }
  DG_REQUIRE((N + 63) / 64 <= 65535, "diagan_attr_dense_wgrad_sgd: N=%d is more than 65535 blocks of 64 rows", N);
  const dim3 grid((K + WG_KSPAN - 1) / WG_KSPAN, (N + 63) / 64);
  hipLaunchKernelGGL(attr_dense_wgrad_kernel, grid, dim3(AT_T), 0, (hipStream_t)stream, dy, y, mask, drop_scale, x, M, K, N, lr,
                     momentum, w, bias, buf_w, buf_b, g_w, g_b);
  return check_launch("diagan_attr_dense_wgrad_sgd");
}

DIAGAN_API int diagan_attr_ce(const float* logits, const int64_t* target, int M, int N, float* dlogit, double* loss_acc,
                              int64_t* correct_acc, void* stream) {
  DG_REQUIRE(logits != nullptr && target != nullptr && dlogit != nullptr && loss_acc != nullptr && correct_acc != nullptr,
             "diagan_attr_ce: null pointer");
  DG_REQUIRE(M >= 1 && N >= 1 && N <= AT_MAX_CLASSES, "diagan_attr_ce: bad shape M=%d N=%d (N <= %d)", M, N, AT_MAX_CLASSES);
  DG_REQUIRE((((uintptr_t)loss_acc | (uintptr_t)correct_acc | (uintptr_t)target) & 7) == 0,
             "diagan_attr_ce: target, loss_acc and correct_acc must be 8-byte aligned");
  hipLaunchKernelGGL(attr_ce_kernel, dim3(1), dim3(AT_T), 0, (hipStream_t)stream, logits, target, M, N, dlogit, loss_acc,
                     correct_acc);
  return check_launch("diagan_attr_ce");
}

DIAGAN_API int diagan_attr_count(const float* logits, int M, int N, int64_t* counter, void* stream) {
  DG_REQUIRE(logits != nullptr && counter != nullptr, "diagan_attr_count: null pointer");
  DG_REQUIRE(M >= 1 && N >= 1 && N <= AT_MAX_CLASSES, "diagan_attr_count: bad shape M=%d N=%d (N <= %d)", M, N, AT_MAX_CLASSES);
  DG_REQUIRE(((uintptr_t)counter & 7) == 0, "diagan_attr_count: counter must be 8-byte aligned");
  hipLaunchKernelGGL(attr_count_kernel, dim3(1), dim3(AT_T), 0, (hipStream_t)stream, logits, M, N, counter);
  return check_launch("diagan_attr_count");
}
