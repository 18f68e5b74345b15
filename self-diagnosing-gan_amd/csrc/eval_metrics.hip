// Evaluation metrics beside FID: the float64 sums of the Kernel Inception Distance and the Inception Score.
//
//   poly_mmd_sums   per subset s of m rows: sxx = sum_{i != j} k(x_i, x_j), syy = sum_{i != j} k(y_i, y_j), sxy = sum_{i, j} k(x_i, y_j)
//                   with k(a, b) = (gamma <a, b> + coef0)^degree.  The dot products run on v_mfma_f64_16x16x4_f64; the power and the
//                   tile's sum are taken in the accumulator registers, so no m x m kernel matrix ever reaches memory.  Rows are
//                   gathered through an index table in the tile loader (no gathered copy of the features).
//   is_scores       per split k of the rows of fp32 logits [N][C]: exp(mean_i sum_c p_ic log p_ic - sum_c pbar_c log pbar_c),
//                   p = softmax(logits) in float64, pbar = the split's column means of p.
//
// Every reduction runs in a fixed order (no float atomics) over caller-owned workspaces: equal inputs give equal bits, and the
// sums of one subset do not depend on what else is in the launch.
#include "common.h"

namespace diagan {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int K_BM = 64, K_BK = 16, K_T = 256;   // the tiling of gemm_f64_kernel (fid_stats.hip): 4 waves, 2 x 2 MFMA tiles each
constexpr int K_LD = K_BM + 16;

__device__ __forceinline__ double ld_feat(const void* p, int is64, long o) {
  return is64 ? ((const double*)p)[o] : (double)((const float*)p)[o];
}

// sum over the K_T threads of a workgroup in a fixed tree: lanes by butterfly, then the waves in order; valid in thread 0
__device__ double block_sum_256(double s, double* red) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < K_T / 64; ++i) t += red[i];
  return t;
}

// grid (T, T, 3 S), T = cdiv(m, 64).  blockIdx.z = 3 s + product (0: xx, 1: yy, 2: xy).  Tile (by, bx) of product p of subset s
// writes ws[((3 s + p) T + by) T + bx]; the symmetric products compute bx >= by only and write 2 x the sum off the diagonal.
__global__ __launch_bounds__(K_T) void poly_mmd_tile_kernel(const void* __restrict__ X, int x64, int Nx, int ldx,
                                                            const void* __restrict__ Y, int y64, int Ny, int ldy,
                                                            const int* __restrict__ idx_x, const int* __restrict__ idx_y, int m, int D,
                                                            int degree, double gamma, double coef0, double* __restrict__ ws) {
  __shared__ double As[K_BK][K_LD];   // As[k][i] = a_{i0 + i}[k0 + k]
  __shared__ double Bs[K_BK][K_LD];   // Bs[k][j] = b_{j0 + j}[k0 + k]
  __shared__ double red[K_T / 64];
  const int prod = blockIdx.z % 3, s = blockIdx.z / 3;
  const bool sym = prod < 2;
  if (sym && blockIdx.x < blockIdx.y) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = (w >> 1) * 32, wn = (w & 1) * 32;
  const int i0 = blockIdx.y * K_BM, j0 = blockIdx.x * K_BM;

  const void* A = prod == 1 ? Y : X;
  const void* B = prod == 0 ? X : Y;
  const int a64 = prod == 1 ? y64 : x64, b64 = prod == 0 ? x64 : y64;
  const int Na = prod == 1 ? Ny : Nx, Nb = prod == 0 ? Nx : Ny;
  const int lda = prod == 1 ? ldy : ldx, ldb = prod == 0 ? ldx : ldy;
  const int* ia = prod == 1 ? idx_y : idx_x;
  const int* ib = prod == 0 ? idx_x : idx_y;

  // thread t loads k = t & 15 of the tile rows (t >> 4) + 16 i, i = 0..3, of both operands; the gathered rows are fixed over K.
  // A row outside the subset or outside its matrix reads as zeros (and is masked out of the sum below).
  long ra_off[4], rb_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (tid >> 4) + 16 * i;
    int ga = -1, gb = -1;
    if (i0 + r < m) ga = ia ? ia[(long)s * m + i0 + r] : i0 + r;
    if (j0 + r < m) gb = ib ? ib[(long)s * m + j0 + r] : j0 + r;
    ra_off[i] = (ga >= 0 && ga < Na) ? (long)ga * lda : -1;
    rb_off[i] = (gb >= 0 && gb < Nb) ? (long)gb * ldb : -1;
  }
  double ra[4], rb[4];
  auto load = [&](int k0) {
    const int gk = k0 + (tid & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = (ra_off[i] >= 0 && gk < D) ? ld_feat(A, a64, ra_off[i] + gk) : 0.0;
      rb[i] = (rb_off[i] >= 0 && gk < D) ? ld_feat(B, b64, rb_off[i] + gk) : 0.0;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      As[tid & 15][(tid >> 4) + 16 * i] = ra[i];
      Bs[tid & 15][(tid >> 4) + 16 * i] = rb[i];
    }
  };

  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  load(0);
  for (int k0 = 0; k0 < D; k0 += K_BK) {
    store();
    __syncthreads();
    if (k0 + K_BK < D) load(k0 + K_BK);
#pragma unroll
    for (int kk = 0; kk < K_BK; kk += 4) {
      const int kr = kk + (lane >> 4), c = lane & 15;
      const double a0 = As[kr][wm + c], a1 = As[kr][wm + 16 + c];
      const double b0 = Bs[kr][wn + c], b1 = Bs[kr][wn + 16 + c];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }

  // the kernel value and the lane's sum, in the accumulator registers; f64 MFMA map: row = (lane >> 4) + 4 r, col = lane & 15
  const bool diag_tile = sym && blockIdx.x == blockIdx.y;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + wm + 16 * i + (lane >> 4) + 4 * r, col = j0 + wn + 16 * j + (lane & 15);
        const double k = gamma * acc[i][j][r] + coef0;
        double p = k;
        for (int d = 1; d < degree; ++d) p *= k;
        if (row < m && col < m && !(diag_tile && row == col)) sum += p;
      }
  sum = block_sum_256(sum, red);
  if (tid == 0) ws[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (sym && !diag_tile) ? 2.0 * sum : sum;
}

// out[3 s + p] = the tile partials of (s, p) in tile order (row-major; the symmetric products' upper triangle only)
__global__ __launch_bounds__(K_T) void poly_mmd_reduce_kernel(const double* __restrict__ ws, int T, double* __restrict__ out) {
  __shared__ double red[K_T / 64];
  const bool sym = blockIdx.x % 3 < 2;
  const double* p = ws + (long)blockIdx.x * T * T;
  double s = 0.0;
  for (int t = threadIdx.x; t < T * T; t += K_T)
    if (!sym || t % T >= t / T) s += p[t];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- Inception Score ----------------------------------------------------------------------------------------------------------------
constexpr int I_CH = 256;   // rows per column-sum chunk (feat_colsum_kernel's pattern)

__device__ __forceinline__ long split_lo(int k, int N, int splits) { return (long)k * N / splits; }

// one wave per row: lse[r] = max + log sum_c exp(l_c - max), h[r] = sum_c p_c log p_c with log p_c = l_c - lse
__global__ __launch_bounds__(256) void is_rows_kernel(const float* __restrict__ logits, int N, int C, int ld, double* __restrict__ lse,
                                                      double* __restrict__ h) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= N) return;
  const float* row = logits + (long)r * ld;
  double mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmax(mx, (double)row[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  double se = 0.0;
  for (int c = lane; c < C; c += 64) se += exp((double)row[c] - mx);
  const double l = mx + log(wave_sum(se));
  double e = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double lp = (double)row[c] - l;
    const double pr = exp(lp);
    if (pr > 0.0) e += pr * lp;   // p = 0 (underflow, or a logit of -inf) contributes 0, not 0 * -inf
  }
  e = wave_sum(e);
  if (lane == 0) {
    lse[r] = l;
    h[r] = e;
  }
}

// part[(k nchunk + chunk) C + c] = sum over the rows of chunk `chunk` of split k, in row order, of p[r][c]
__global__ __launch_bounds__(256) void is_colsum_kernel(const float* __restrict__ logits, const double* __restrict__ lse, int N, int C,
                                                        int ld, int splits, int nchunk, double* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x, k = blockIdx.z;
  if (c >= C) return;
  const long lo = split_lo(k, N, splits), hi = split_lo(k + 1, N, splits);
  const long r0 = lo + (long)blockIdx.y * I_CH, r1 = min(hi, r0 + I_CH);
  double s = 0.0;
  for (long r = r0; r < r1; ++r) s += exp((double)logits[r * ld + c] - lse[r]);
  part[((long)k * nchunk + blockIdx.y) * C + c] = s;
}

// one workgroup per split: score = exp(mean_i h_i - sum_c pbar_c log pbar_c), 0 log 0 = 0
__global__ __launch_bounds__(K_T) void is_final_kernel(const double* __restrict__ part, const double* __restrict__ h, int N, int C,
                                                       int splits, int nchunk, double* __restrict__ out) {
  __shared__ double red[K_T / 64];
  const int k = blockIdx.x;
  const long lo = split_lo(k, N, splits), hi = split_lo(k + 1, N, splits);
  const double n = (double)(hi - lo);
  double sh = 0.0;
  for (long r = lo + threadIdx.x; r < hi; r += K_T) sh += h[r];
  sh = block_sum_256(sh, red);
  __syncthreads();
  double sp = 0.0;
  for (int c = threadIdx.x; c < C; c += K_T) {
    double t = 0.0;
    for (int j = 0; j < nchunk; ++j) t += part[((long)k * nchunk + j) * C + c];
    const double pbar = t / n;
    if (pbar > 0.0) sp += pbar * log(pbar);
  }
  sp = block_sum_256(sp, red);
  if (threadIdx.x == 0) out[k] = exp(sh / n - sp);
}

static inline int is_nchunk(int N, int splits) {   // chunks of the longest split: lengths are floor(N / splits) or one more
  return cdiv(cdiv(N, splits), I_CH);
}

}  // namespace diagan

using namespace diagan;

DIAGAN_API int diagan_poly_mmd_ws(int m) {   // doubles of workspace per subset
  if (m <= 0) return -1;
  const int64_t T = cdiv(m, K_BM);
  return 3 * T * T <= INT32_MAX ? (int)(3 * T * T) : -1;
}

DIAGAN_API int diagan_poly_mmd_sums(const void* X, int x_f64, int Nx, int ldx, const void* Y, int y_f64, int Ny, int ldy, const int* idx_x,
                                    const int* idx_y, int S, int m, int D, int degree, double gamma, double coef0, double* ws,
                                    double* out, void* stream) {
  DG_REQUIRE(X && Y && ws && out && S > 0 && m > 0 && D > 0 && Nx > 0 && Ny > 0, "poly_mmd_sums: bad args");
  DG_REQUIRE(ldx >= D && ldy >= D, "poly_mmd_sums: leading dimensions too small");
  DG_REQUIRE(degree >= 1, "poly_mmd_sums: degree must be >= 1");
  DG_REQUIRE((idx_x || m <= Nx) && (idx_y || m <= Ny), "poly_mmd_sums: without an index table the subset is rows 0..m-1");
  const int T = cdiv(m, K_BM);
  DG_REQUIRE(T <= 65535 && 3L * S <= 65535, "poly_mmd_sums: %d tiles x %d subsets exceed the launch grid", T, S);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(poly_mmd_tile_kernel, dim3(T, T, 3 * S), dim3(K_T), 0, st, X, x_f64, Nx, ldx, Y, y_f64, Ny, ldy, idx_x, idx_y, m, D,
                     degree, gamma, coef0, ws);
  hipLaunchKernelGGL(poly_mmd_reduce_kernel, dim3(3 * S), dim3(K_T), 0, st, ws, T, out);
  return check_launch("poly_mmd_sums");
}

DIAGAN_API int diagan_is_ws(int N, int C, int splits) {   // doubles of workspace
  if (N <= 0 || C <= 0 || splits <= 0 || splits > N) return -1;
  if (is_nchunk(N, splits) > 65535) return -1;   // the chunks of a split are a grid dimension
  const int64_t n = 2 * (int64_t)N + (int64_t)splits * is_nchunk(N, splits) * C;
  return n <= INT32_MAX ? (int)n : -1;
}

DIAGAN_API int diagan_is_scores(const float* logits, int N, int C, int ld, int splits, double* ws, double* out, void* stream) {
  DG_REQUIRE(logits && ws && out && N > 0 && C > 0 && ld >= C, "is_scores: bad args");
  DG_REQUIRE(splits > 0 && splits <= N && splits <= 65535, "is_scores: %d splits of %d rows", splits, N);
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = is_nchunk(N, splits);
  DG_REQUIRE(nchunk <= 65535, "is_scores: %d row chunks per split exceed the launch grid (use more splits)", nchunk);
  double *lse = ws, *h = ws + N, *part = ws + 2 * (long)N;
  hipLaunchKernelGGL(is_rows_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, logits, N, C, ld, lse, h);
  hipLaunchKernelGGL(is_colsum_kernel, dim3(cdiv(C, 256), nchunk, splits), dim3(256), 0, st, logits, lse, N, C, ld, splits, nchunk, part);
  hipLaunchKernelGGL(is_final_kernel, dim3(splits), dim3(K_T), 0, st, part, h, N, C, splits, nchunk, out);
  return check_launch("is_scores");
}
