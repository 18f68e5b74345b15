// FID in feature space: the float64 arithmetic of diagan-pkg/diagan/trainer/fid_utils.py on the device.
//
//   gemm_f64           C = alpha * op(A) B + beta * C + diag * I on v_mfma_f64_16x16x4_f64; optional per-tile partial traces
//   feat_row_mask      ~isnan(act).any(1) & ~isinf(act).any(1)                     (fid_utils.py:87-88)
//   feat_colsum / feat_mean / feat_center
//                      np.mean(act, axis=0) and the centred rows of np.cov          (fid_utils.py:90-91)
//   moments_merge      Chan's parallel update of (n, mean, M2) by one batch
//   sym_f64 / trace_f64 / scale_diag_f64 / sum_f64 / fid_term
//                      the small pieces of calculate_frechet_distance              (fid_utils.py:11-67)
//
// Every reduction runs in a fixed order (no float atomics): two runs give the same bits.
#include "common.h"

namespace diagan {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- fp64 GEMM ------------------------------------------------------------------------------------------------------------------
// 64 x 64 output tile per workgroup, 4 waves in a 2 x 2 grid of 32 x 32, each wave 2 x 2 MFMA tiles of 16 x 16; K in steps of 16
// through LDS, the next step's global loads held in registers while the current one is multiplied.
// MFMA f64 16x16x4 operands (one double per lane): A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15];
// result register r of lane l is C[row = (l >> 4) + 4 r][col = l & 15]: NOT the fp32 16x16 map (row = 4 (l >> 4) + r).
constexpr int G_BM = 64, G_BK = 16, G_T = 256;
constexpr int G_LD = G_BM + 16;   // 640-byte LDS rows: the two 16-lane k rows a half-wave reads land in disjoint banks

template <bool TRANS_A>
__global__ __launch_bounds__(G_T) void gemm_f64_kernel(const double* __restrict__ A, const double* __restrict__ B, double* C, int M,
                                                       int N, int K, int lda, int ldb, int ldc, double alpha, double beta, double diag,
                                                       double* __restrict__ trace_part) {
  __shared__ double As[G_BK][G_LD];   // As[k][m] = op(A)[m0 + m][k0 + k]
  __shared__ double Bs[G_BK][G_LD];   // Bs[k][n] = B[k0 + k][n0 + n]
  __shared__ double dg[G_BM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = (w >> 1) * 32, wn = (w & 1) * 32;
  const int m0 = blockIdx.y * G_BM, n0 = blockIdx.x * G_BM;
  if (tid < G_BM) dg[tid] = 0.0;

  double ra[4], rb[4];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + G_T * i;
      int m, k;
      if (TRANS_A) { k = idx >> 6; m = idx & 63; }   // A is [K][M]: coalesced along m
      else { m = idx >> 4; k = idx & 15; }           // A is [M][K]: 16 consecutive k per row
      const int gm = m0 + m, gk = k0 + k;
      ra[i] = (gm < M && gk < K) ? (TRANS_A ? A[(long)gk * lda + gm] : A[(long)gm * lda + gk]) : 0.0;
      const int gkb = k0 + (idx >> 6), gn = n0 + (idx & 63);
      rb[i] = (gkb < K && gn < N) ? B[(long)gkb * ldb + gn] : 0.0;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + G_T * i;
      if (TRANS_A) As[idx >> 6][idx & 63] = ra[i];
      else As[idx & 15][idx >> 4] = ra[i];
      Bs[idx >> 6][idx & 63] = rb[i];
    }
  };

  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  load(0);
  for (int k0 = 0; k0 < K; k0 += G_BK) {
    store();
    __syncthreads();
    if (k0 + G_BK < K) load(k0 + G_BK);
#pragma unroll
    for (int kk = 0; kk < G_BK; kk += 4) {
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

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + 16 * i + (lane >> 4) + 4 * r, col = n0 + wn + 16 * j + (lane & 15);
        if (row < M && col < N) {
          double v = alpha * acc[i][j][r];
          if (beta != 0.0) v += beta * C[(long)row * ldc + col];   // beta == 0: C is not read (may be uninitialised)
          if (row == col) {
            v += diag;
            dg[row - m0] = v;
          }
          C[(long)row * ldc + col] = v;
        }
      }
  if (trace_part && blockIdx.x == blockIdx.y) {   // a diagonal tile: its partial trace, summed in row order
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int i = 0; i < G_BM; ++i) s += dg[i];
      trace_part[blockIdx.y] = s;
    }
  }
}

// ---- fixed-order reductions -----------------------------------------------------------------------------------------------------
constexpr int R_T = 1024;

__device__ double block_sum_fixed(double s, double* red) {   // R_T threads; same tree every call
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < R_T / 64; ++i) t += red[i];
  return t;
}

// out[0] = sum x[i] (square: sum x[i]^2), one workgroup
__global__ __launch_bounds__(R_T) void sum_f64_kernel(const double* __restrict__ x, long n, int square, double* __restrict__ out) {
  __shared__ double red[R_T / 64];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += R_T) {
    const double v = x[i];
    s += square ? v * v : v;
  }
  s = block_sum_fixed(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

__global__ __launch_bounds__(R_T) void trace_f64_kernel(const double* __restrict__ S, int D, int ld, double* __restrict__ out) {
  __shared__ double red[R_T / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < D; i += R_T) s += S[(long)i * ld + i];
  s = block_sum_fixed(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

// out[0] = |mu1 - mu2|^2 + tr S1 + tr S2
__global__ __launch_bounds__(R_T) void fid_term_kernel(const double* __restrict__ mu1, const double* __restrict__ mu2,
                                                       const double* __restrict__ S1, const double* __restrict__ S2, int D, int ld,
                                                       double* __restrict__ out) {
  __shared__ double red[R_T / 64];
  double d2 = 0.0, t1 = 0.0, t2 = 0.0;
  for (int i = threadIdx.x; i < D; i += R_T) {
    const double d = mu1[i] - mu2[i];
    d2 += d * d;
    t1 += S1[(long)i * ld + i];
    t2 += S2[(long)i * ld + i];
  }
  d2 = block_sum_fixed(d2, red);
  __syncthreads();
  t1 = block_sum_fixed(t1, red);
  __syncthreads();
  t2 = block_sum_fixed(t2, red);
  if (threadIdx.x == 0) out[0] = d2 + t1 + t2;
}

// ---- element-wise matrix pieces ---------------------------------------------------------------------------------------------------
constexpr int E_T = 16;   // 16 x 16 threads

// S = scale * (S + S^T) / 2 in place: the thread of (i, j), j >= i, owns both mirror elements
__global__ __launch_bounds__(E_T* E_T) void sym_f64_kernel(double* S, int D, int ld, double scale) {
  const int j = blockIdx.x * E_T + threadIdx.x, i = blockIdx.y * E_T + threadIdx.y;
  if (i >= D || j >= D || j < i) return;
  const double v = 0.5 * (S[(long)i * ld + j] + S[(long)j * ld + i]) * scale;
  S[(long)i * ld + j] = v;
  S[(long)j * ld + i] = v;
}

// dst = alpha * src + d * I   (src NULL: dst = d * I)
__global__ __launch_bounds__(E_T* E_T) void scale_diag_f64_kernel(const double* src, double* dst, int D, int ld, double alpha, double d) {
  const int j = blockIdx.x * E_T + threadIdx.x, i = blockIdx.y * E_T + threadIdx.y;
  if (i >= D || j >= D) return;
  double v = src ? alpha * src[(long)i * ld + j] : 0.0;
  if (i == j) v += d;
  dst[(long)i * ld + j] = v;
}

// ---- feature moments --------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ double ld64(const T* p) { return (double)*p; }

// mask[r] = 1.0 when every element of row r is finite, else 0.0; one wave per row
template <typename T>
__global__ __launch_bounds__(256) void feat_row_mask_kernel(const T* __restrict__ x, int N, int D, int ld, double* __restrict__ mask) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= N) return;
  bool ok = true;
  for (int c = lane; c < D; c += 64) ok &= __builtin_isfinite(ld64(x + (long)r * ld + c));
  ok = __all(ok);
  if (lane == 0) mask[r] = ok ? 1.0 : 0.0;
}

constexpr int M_CH = 256;   // rows per column-sum chunk

// part[chunk][c] = sum over the kept rows of the chunk (in row order) of x[r][c]
template <typename T>
__global__ __launch_bounds__(256) void feat_colsum_kernel(const T* __restrict__ x, const double* __restrict__ mask, int N, int D, int ld,
                                                          double* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * M_CH;
  if (c >= D) return;
  const int r1 = min(N, r0 + M_CH);
  double s = 0.0;
  for (int r = r0; r < r1; ++r)
    if (mask[r] != 0.0) s += ld64(x + (long)r * ld + c);
  part[(long)blockIdx.y * D + c] = s;
}

// mean[c] = sum_chunk part[chunk][c] / count[0]  (0 when no row was kept)
__global__ __launch_bounds__(256) void feat_mean_kernel(const double* __restrict__ part, int nchunk, const double* __restrict__ count,
                                                        int D, double* __restrict__ mean) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  double s = 0.0;
  for (int k = 0; k < nchunk; ++k) s += part[(long)k * D + c];
  const double n = count[0];
  mean[c] = n > 0.0 ? s / n : 0.0;
}

// xc[r][c] = x[r][c] - mean[c] for kept rows, 0 for dropped ones (they add nothing to Xc^T Xc)
template <typename T>
__global__ __launch_bounds__(256) void feat_center_kernel(const T* __restrict__ x, const double* __restrict__ mask,
                                                          const double* __restrict__ mean, int N, int D, int ld, double* __restrict__ xc,
                                                          int ldc) {
  const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (c >= D) return;
  xc[(long)r * ldc + c] = mask[r] != 0.0 ? ld64(x + (long)r * ld + c) - mean[c] : 0.0;
}

// Chan et al.: n = na + nb, delta = mean_b - mean_a, M2 = M2_a + M2_b + delta delta^T na nb / n, mean = mean_a + delta nb / n.
// The M2 kernel reads the old means, so it runs first; the second kernel (one workgroup) updates the means, then the count.
__global__ __launch_bounds__(E_T* E_T) void merge_m2_kernel(const double* __restrict__ n_run, const double* __restrict__ mean_run,
                                                            double* __restrict__ m2_run, int ld, const double* __restrict__ n_b,
                                                            const double* __restrict__ mean_b, const double* __restrict__ m2_b, int ldb,
                                                            int D) {
  const int j = blockIdx.x * E_T + threadIdx.x, i = blockIdx.y * E_T + threadIdx.y;
  if (i >= D || j >= D) return;
  const double na = n_run[0], nb = n_b[0];
  if (nb == 0.0) return;
  const double f = na * nb / (na + nb);
  m2_run[(long)i * ld + j] += m2_b[(long)i * ldb + j] + f * (mean_b[i] - mean_run[i]) * (mean_b[j] - mean_run[j]);
}

__global__ __launch_bounds__(256) void merge_mean_kernel(double* __restrict__ n_run, double* __restrict__ mean_run,
                                                         const double* __restrict__ n_b, const double* __restrict__ mean_b, int D) {
  const double na = n_run[0], nb = n_b[0];
  if (nb == 0.0) return;
  const double f = nb / (na + nb);
  for (int c = threadIdx.x; c < D; c += 256) mean_run[c] += (mean_b[c] - mean_run[c]) * f;
  __syncthreads();
  if (threadIdx.x == 0) n_run[0] = na + nb;
}

}  // namespace diagan

using namespace diagan;

DIAGAN_API int diagan_gemm_f64(const double* A, const double* B, double* C, int M, int N, int K, int lda, int ldb, int ldc, int trans_a,
                               double alpha, double beta, double diag, double* trace_part, void* stream) {
  DG_REQUIRE(A && B && C && M > 0 && N > 0 && K > 0, "gemm_f64: bad args");
  DG_REQUIRE(lda >= (trans_a ? M : K) && ldb >= N && ldc >= N, "gemm_f64: leading dimensions too small");
  DG_REQUIRE(!trace_part || M == N, "gemm_f64: partial traces need a square C");
  DG_REQUIRE(C != A && C != B, "gemm_f64: C must not alias an operand");
  const dim3 grid(cdiv(N, G_BM), cdiv(M, G_BM));
  if (trans_a)
    hipLaunchKernelGGL(gemm_f64_kernel<true>, grid, dim3(G_T), 0, (hipStream_t)stream, A, B, C, M, N, K, lda, ldb, ldc, alpha, beta, diag,
                       trace_part);
  else
    hipLaunchKernelGGL(gemm_f64_kernel<false>, grid, dim3(G_T), 0, (hipStream_t)stream, A, B, C, M, N, K, lda, ldb, ldc, alpha, beta, diag,
                       trace_part);
  return check_launch("gemm_f64");
}

DIAGAN_API int diagan_gemm_f64_tile(void) { return G_BM; }

DIAGAN_API int diagan_sum_f64(const double* x, int64_t n, int square, double* out, void* stream) {
  DG_REQUIRE(x && out && n > 0, "sum_f64: bad args");
  hipLaunchKernelGGL(sum_f64_kernel, dim3(1), dim3(R_T), 0, (hipStream_t)stream, x, (long)n, square, out);
  return check_launch("sum_f64");
}

DIAGAN_API int diagan_trace_f64(const double* S, int D, int ld, double* out, void* stream) {
  DG_REQUIRE(S && out && D > 0 && ld >= D, "trace_f64: bad args");
  hipLaunchKernelGGL(trace_f64_kernel, dim3(1), dim3(R_T), 0, (hipStream_t)stream, S, D, ld, out);
  return check_launch("trace_f64");
}

DIAGAN_API int diagan_sym_f64(double* S, int D, int ld, double scale, void* stream) {
  DG_REQUIRE(S && D > 0 && ld >= D, "sym_f64: bad args");
  hipLaunchKernelGGL(sym_f64_kernel, dim3(cdiv(D, E_T), cdiv(D, E_T)), dim3(E_T, E_T), 0, (hipStream_t)stream, S, D, ld, scale);
  return check_launch("sym_f64");
}

DIAGAN_API int diagan_scale_diag_f64(const double* src, double* dst, int D, int ld, double alpha, double d, void* stream) {
  DG_REQUIRE(dst && D > 0 && ld >= D, "scale_diag_f64: bad args");
  hipLaunchKernelGGL(scale_diag_f64_kernel, dim3(cdiv(D, E_T), cdiv(D, E_T)), dim3(E_T, E_T), 0, (hipStream_t)stream, src, dst, D, ld,
                     alpha, d);
  return check_launch("scale_diag_f64");
}

DIAGAN_API int diagan_fid_term(const double* mu1, const double* mu2, const double* S1, const double* S2, int D, int ld, double* out,
                               void* stream) {
  DG_REQUIRE(mu1 && mu2 && S1 && S2 && out && D > 0 && ld >= D, "fid_term: bad args");
  hipLaunchKernelGGL(fid_term_kernel, dim3(1), dim3(R_T), 0, (hipStream_t)stream, mu1, mu2, S1, S2, D, ld, out);
  return check_launch("fid_term");
}

DIAGAN_API int diagan_feat_colsum_chunks(int N) { return cdiv(N, M_CH); }

DIAGAN_API int diagan_feat_moments(const void* x, int x_f64, int N, int D, int ld, double* mask, double* part, double* count, double* mean,
                                   void* stream) {
  DG_REQUIRE(x && mask && part && count && mean && N > 0 && D > 0 && ld >= D, "feat_moments: bad args");
  hipStream_t s = (hipStream_t)stream;
  const dim3 gc(cdiv(D, 256), cdiv(N, M_CH));
  if (x_f64) {
    hipLaunchKernelGGL(feat_row_mask_kernel<double>, dim3(cdiv(N, 4)), dim3(256), 0, s, (const double*)x, N, D, ld, mask);
    hipLaunchKernelGGL(feat_colsum_kernel<double>, gc, dim3(256), 0, s, (const double*)x, mask, N, D, ld, part);
  } else {
    hipLaunchKernelGGL(feat_row_mask_kernel<float>, dim3(cdiv(N, 4)), dim3(256), 0, s, (const float*)x, N, D, ld, mask);
    hipLaunchKernelGGL(feat_colsum_kernel<float>, gc, dim3(256), 0, s, (const float*)x, mask, N, D, ld, part);
  }
  hipLaunchKernelGGL(sum_f64_kernel, dim3(1), dim3(R_T), 0, s, mask, (long)N, 0, count);
  hipLaunchKernelGGL(feat_mean_kernel, dim3(cdiv(D, 256)), dim3(256), 0, s, part, (int)gc.y, count, D, mean);
  return check_launch("feat_moments");
}

DIAGAN_API int diagan_feat_center(const void* x, int x_f64, const double* mask, const double* mean, int N, int D, int ld, double* xc,
                                  int ldc, void* stream) {
  DG_REQUIRE(x && mask && mean && xc && N > 0 && D > 0 && ld >= D && ldc >= D, "feat_center: bad args");
  const dim3 g(cdiv(D, 256), N);
  if (x_f64)
    hipLaunchKernelGGL(feat_center_kernel<double>, g, dim3(256), 0, (hipStream_t)stream, (const double*)x, mask, mean, N, D, ld, xc, ldc);
  else
    hipLaunchKernelGGL(feat_center_kernel<float>, g, dim3(256), 0, (hipStream_t)stream, (const float*)x, mask, mean, N, D, ld, xc, ldc);
  return check_launch("feat_center");
}

DIAGAN_API int diagan_moments_merge(double* n_run, double* mean_run, double* m2_run, int ld, const double* n_b, const double* mean_b,
                                    const double* m2_b, int ldb, int D, void* stream) {
  DG_REQUIRE(n_run && mean_run && m2_run && n_b && mean_b && m2_b && D > 0 && ld >= D && ldb >= D, "moments_merge: bad args");
  hipLaunchKernelGGL(merge_m2_kernel, dim3(cdiv(D, E_T), cdiv(D, E_T)), dim3(E_T, E_T), 0, (hipStream_t)stream, n_run, mean_run, m2_run,
                     ld, n_b, mean_b, m2_b, ldb, D);
  hipLaunchKernelGGL(merge_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_run, mean_run, n_b, mean_b, D);
  return check_launch("moments_merge");
}
