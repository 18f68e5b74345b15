// Nearest-row search in feature space: for every query row r the candidate j that minimises
//     t[r][j] = |c_j|^2 - 2 <q_r, c_j>
// (the squared distance without its row term |q_r|^2, which is constant in j), as a GEMM whose epilogue keeps the running
// (minimum, index) pair -- no Nq x Nc matrix ever reaches memory.  The nearest-latent refresh of the Inclusive GAN baseline
// (diagan-pkg/diagan/models/inclusive_gan.py:178-199) is this search.
//
//   nn_argmin_tile    128 queries x 128 candidates per K loop on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation),
//                     both operands staged through LDS, the last K step masked (any D, no padded copy).  A workgroup walks the
//                     candidate tiles of its split (gridDim.y splits of the candidate axis) with one (value, index) pair per
//                     accumulator element, reduces each row over the lanes and then over the waves, and writes one pair per
//                     (query, split) to the caller's workspace.
//   nn_argmin_merge   one thread per query: the splits in order, then (accumulate) what the caller already holds.
//
// t[r][j] is computed by one lane in a K order (pieces of NN_KC columns, summed in order) that depends on neither the tile nor the split, and a minimum rounds nothing:
// best_t and best_idx are the same bits for any split count and for candidates fed in one call or in several.  Among bit-equal
// values the lowest global index wins everywhere (per lane by strict <, across lanes, waves and splits by comparing indices).
// No float atomics, no allocation.
#include "common.h"

#include <limits.h>

namespace diagan {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// 4 waves in a 2 (queries) x 2 (candidates) grid, each wave 64 x 64 = four 32 x 32 accumulators.  MFMA 32x32x2 f32 operands:
// A[row = lane & 31][k = lane >> 5] (a query), B[k = lane >> 5][col = lane & 31] (a candidate); result register e of lane l is
// C[row = 4 (l >> 5) + (e & 3) + 8 (e >> 2)][col = l & 31].  The next K-step's global loads are held in registers while the
// current one is multiplied.
constexpr int NN_BM = 128, NN_BN = 128, NN_BK = 16, NN_T = 256;
constexpr int NN_KC = 128;                // the MFMA chain of one dot product is cut every NN_KC columns (see the K loop)
constexpr int NN_LD = NN_BM + 4;          // row stride 4 banks off a multiple of 32: the four k-groups of a store land apart
constexpr int NN_TARGET_WGS = 2048;       // about four rounds of two workgroups per CU on 256 CUs
constexpr int NN_MAX_SPLITS = 4096;

__device__ __forceinline__ bool nn_better(float v, int i, float bv, int bi) { return v < bv || (v == bv && i < bi); }

template <bool VEC>
__global__ __launch_bounds__(NN_T) void nn_argmin_tile_kernel(const float* __restrict__ q, int Nq, int ldq,
                                                              const float* __restrict__ c, int Nc, int ldc,
                                                              const float* __restrict__ cn, int D, int tiles_per_split,
                                                              float* __restrict__ ws_t, int* __restrict__ ws_i) {
  __shared__ float As[NN_BK][NN_LD];      // As[k][m]: the tile's queries
  __shared__ float Bs[NN_BK][NN_LD];      // Bs[k][n]: the tile's candidates
  __shared__ float red_t[2][NN_BM];       // per candidate-side wave: the row's pair
  __shared__ int red_i[2][NN_BM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fi = lane & 31, fh = lane >> 5;
  const int wm = (w & 1) * 64, wn = (w >> 1) * 64;
  const int kg = tid & 3, lr = tid >> 2;  // this thread's k-group of 4 in every K-step and its tile rows lr, lr + 64
  const int m0 = blockIdx.x * NN_BM;
  const int ntiles = (Nc + NN_BN - 1) / NN_BN;
  const int t_lo = blockIdx.y * tiles_per_split;
  const int t_hi = min(ntiles, t_lo + tiles_per_split);

  const float* qrow[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = m0 + lr + 64 * j;
    qrow[j] = r < Nq ? q + (long)r * ldq : nullptr;
  }
  auto ld4 = [&](const float* row, int k) -> f32x4 {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row == nullptr || k >= D) return v;
    if (VEC && k + 4 <= D) return *reinterpret_cast<const f32x4*>(row + k);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < D) v[e] = row[k + e];
    return v;
  };

  float best_t[2][16];
  int best_i[2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      best_t[i][e] = INFINITY;
      best_i[i][e] = INT_MAX;
    }

  for (int t = t_lo; t < t_hi; ++t) {
    const int n0 = t * NN_BN;
    const float* crow[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = n0 + lr + 64 * j;
      crow[j] = r < Nc ? c + (long)r * ldc : nullptr;
    }
    f32x4 ra[2], rb[2];
    auto load = [&](int k0) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        ra[j] = ld4(qrow[j], k0 + 4 * kg);
        rb[j] = ld4(crow[j], k0 + 4 * kg);
      }
    };
    auto store = [&]() {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          As[4 * kg + e][lr + 64 * j] = ra[j][e];
          Bs[4 * kg + e][lr + 64 * j] = rb[j][e];
        }
    };

    // A dot product over D = 2048 as one chain of 1024 MFMA steps rounds into partial sums that grow to the size of the
    // result; measured against float64 that is twice the error of a blocked fp32 GEMM.  So acc holds NN_KC columns at a time
    // and dot collects the pieces: the partial sums inside a piece stay small, and only D / NN_KC additions see the full size.
    f32x16 acc[2][2], dot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = dot[i][j][e] = 0.f;

    load(0);
    for (int k0 = 0; k0 < D; k0 += NN_BK) {
      store();
      __syncthreads();
      if (k0 + NN_BK < D) load(k0 + NN_BK);
#pragma unroll
      for (int s = 0; s < NN_BK / 2; ++s) {
        const int kr = 2 * s + fh;
        const float a0 = As[kr][wm + fi], a1 = As[kr][wm + 32 + fi];
        const float b0 = Bs[kr][wn + fi], b1 = Bs[kr][wn + 32 + fi];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      if ((k0 + NN_BK) % NN_KC == 0 || k0 + NN_BK >= D) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              dot[i][j][e] += acc[i][j][e];
              acc[i][j][e] = 0.f;
            }
      }
      __syncthreads();
    }

    // |c|^2 - 2 q.c against this lane's running pairs; a lane meets its columns in ascending order, so strict < keeps the lowest
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn + 32 * j + fi;
      if (col < Nc) {
        const float cv = cn[col];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float v = cv - 2.f * dot[i][j][e];
            if (v < best_t[i][e]) {
              best_t[i][e] = v;
              best_i[i][e] = col;
            }
          }
      }
    }
  }

  // each row over the 32 lanes that hold it (the exchange stays inside a half-wave), then over the two candidate-side waves
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float v = best_t[i][e];
      int ix = best_i[i][e];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(ix, o, 64);
        if (nn_better(ov, oi, v, ix)) {
          v = ov;
          ix = oi;
        }
      }
      if (fi == 0) {
        const int row = wm + 32 * i + 4 * fh + (e & 3) + 8 * (e >> 2);
        red_t[w >> 1][row] = v;
        red_i[w >> 1][row] = ix;
      }
    }
  __syncthreads();
  if (tid < NN_BM && m0 + tid < Nq) {
    float v = red_t[0][tid];
    int ix = red_i[0][tid];
    if (nn_better(red_t[1][tid], red_i[1][tid], v, ix)) {
      v = red_t[1][tid];
      ix = red_i[1][tid];
    }
    const long o = (long)blockIdx.y * Nq + m0 + tid;
    ws_t[o] = v;
    ws_i[o] = ix;
  }
}

// The splits hold ascending, disjoint index ranges; what the caller already holds (accumulate) has lower indices than this call's
// candidates, so it is replaced on strict < only.  A query for which no t compared below +inf (inputs that are not finite) gets
// this call's first candidate, so that the index stays in range.
__global__ __launch_bounds__(256) void nn_argmin_merge_kernel(const float* __restrict__ ws_t, const int* __restrict__ ws_i, int Nq,
                                                              int splits, long idx_offset, int accumulate, float* __restrict__ best_t,
                                                              long* __restrict__ best_idx) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= Nq) return;
  float v = ws_t[r];
  int ix = ws_i[r];
  for (int s = 1; s < splits; ++s) {
    const float ov = ws_t[(long)s * Nq + r];
    const int oi = ws_i[(long)s * Nq + r];
    if (nn_better(ov, oi, v, ix)) {
      v = ov;
      ix = oi;
    }
  }
  if (ix == INT_MAX) ix = 0;
  if (accumulate && !(v < best_t[r])) return;
  best_t[r] = v;
  best_idx[r] = idx_offset + ix;
}

// how the candidate tiles are cut: a function of the shape alone (the workspace query and the launch agree)
static inline void nn_plan(int Nq, int Nc, int* splits, int* tiles_per_split) {
  const int rb = cdiv(Nq, NN_BM), ntiles = cdiv(Nc, NN_BN);
  int want = NN_TARGET_WGS / rb;
  want = want < 1 ? 1 : (want > NN_MAX_SPLITS ? NN_MAX_SPLITS : want);
  if (want > ntiles) want = ntiles;
  *tiles_per_split = cdiv(ntiles, want);
  *splits = cdiv(ntiles, *tiles_per_split);      // every split holds at least one tile
}

}  // namespace diagan

using namespace diagan;

DIAGAN_API size_t diagan_nn_argmin_ws(int Nq, int Nc) {   // bytes of workspace; 0 for a bad shape
  if (Nq <= 0 || Nc <= 0) return 0;
  int splits, tps;
  nn_plan(Nq, Nc, &splits, &tps);
  return (size_t)splits * (size_t)Nq * (sizeof(float) + sizeof(int));
}

DIAGAN_API int diagan_nn_argmin(const float* q, int Nq, int ldq, const float* c, int Nc, int ldc, const float* c_sqnorm, int D,
                                long idx_offset, int accumulate, float* best_t, long* best_idx, void* ws, void* stream) {
  DG_REQUIRE(q && c && c_sqnorm && best_t && best_idx && ws, "nn_argmin: NULL pointer");
  DG_REQUIRE(Nq > 0 && Nc > 0, "nn_argmin: %d queries, %d candidates (both must be positive)", Nq, Nc);
  DG_REQUIRE(D > 0, "nn_argmin: feature width D = %d must be positive", D);
  DG_REQUIRE(ldq >= D && ldc >= D, "nn_argmin: leading dimensions %d, %d smaller than D = %d", ldq, ldc, D);
  DG_REQUIRE(idx_offset >= 0, "nn_argmin: negative index offset");
  DG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "nn_argmin: the workspace must be 4-byte aligned");
  int splits, tps;
  nn_plan(Nq, Nc, &splits, &tps);
  const int rb = cdiv(Nq, NN_BM);
  float* ws_t = (float*)ws;
  int* ws_i = (int*)(ws_t + (size_t)splits * Nq);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = ldq % 4 == 0 && ldc % 4 == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(c) & 15) == 0;
  if (vec)
    nn_argmin_tile_kernel<true><<<dim3(rb, splits), NN_T, 0, st>>>(q, Nq, ldq, c, Nc, ldc, c_sqnorm, D, tps, ws_t, ws_i);
  else
    nn_argmin_tile_kernel<false><<<dim3(rb, splits), NN_T, 0, st>>>(q, Nq, ldq, c, Nc, ldc, c_sqnorm, D, tps, ws_t, ws_i);
  nn_argmin_merge_kernel<<<cdiv(Nq, 256), 256, 0, st>>>(ws_t, ws_i, Nq, splits, idx_offset, accumulate ? 1 : 0, best_t, best_idx);
  return check_launch("nn_argmin");
}
