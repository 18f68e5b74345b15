// Precision / recall / density / coverage (Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative Models", ICML 2020)
// from ONE read of a block of the pairwise-distance matrix: the four reductions of include/diagan_prdc.h, DESIGN §8k.
// pr_metrics.hip's any_lt_rows / any_lt_cols each read the block once for one flag; coverage needs the minimum over a row and
// density a count over a column, and a group diagnostic needs the per-sample vectors of all of them.
//
//   prdc_tile_kernel    workgroup = 64 rows x 1024 columns of T.  A lane owns 4 consecutive columns (one 16-byte load per row, a
//                       wave reads 1 KiB contiguous): its 4 column counts live in registers over the 64 rows; per row the
//                       wave's minimum comes from shuffles and its hit flag from a ballot, the 4 waves meet in LDS.
//                       Row partials go to ws per COLUMN tile, column counts per ROW tile.
//   prdc_finish_kernel  combines the partials: min / OR over the column tiles, integer sum over the row tiles
//                       (col_hit = count > 0), merging into the outputs when `accumulate`.
// No atomics; min, OR and integer sums are exact in any order, so the outputs do not depend on the tiling or the launch geometry.
//
// Roofline: HBM.  T is read once (N = 10 000: 400 MB); per 16 bytes loaded a lane does 4 adds, 4 mins and 8 compares, and the
// workspace traffic is cols * 4 bytes per 64 rows written and read back: 1/64 of T each way.
#include "common.h"
#include "diagan_prdc.h"

namespace diagan {

typedef float prdc_f32x4 __attribute__((ext_vector_type(4)));
constexpr int PD_T = 256;            // threads per workgroup (4 waves)
constexpr int PD_TR = 64;            // rows per tile
constexpr int PD_TC = PD_T * 4;      // columns per tile
constexpr int PD_U = 4;              // rows in flight per lane

__device__ __forceinline__ float prdc_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(PD_T) void prdc_tile_kernel(const float* __restrict__ T, const float* __restrict__ row_add,
                                                         const float* __restrict__ thr_col, const float* __restrict__ thr_row,
                                                         int rows, int cols, long ld, float* __restrict__ ws_min,
                                                         int* __restrict__ ws_hit, int* __restrict__ ws_cnt) {
  __shared__ float smin[4][PD_TR];
  __shared__ int shit[4][PD_TR];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long c0 = (long)blockIdx.x * PD_TC + tid * 4;
  const int r0 = blockIdx.y * PD_TR;
  const int r1 = min(r0 + PD_TR, rows);
  const float inf = __builtin_huge_valf();
  const bool full = c0 + 3 < cols;                      // all 4 columns of this lane exist
  float tc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) tc[j] = c0 + j < cols ? thr_col[c0 + j] : -inf;      // a missing column never hits
  int cnt[4] = {0, 0, 0, 0};
  for (int rb = r0; rb < r1; rb += PD_U) {
    float v[PD_U][4];
#pragma unroll
    for (int u = 0; u < PD_U; ++u) {
      const int r = min(rb + u, r1 - 1);                // clamped: the load stays inside the block, the row is skipped below
      const float* p = T + (long)r * ld + c0;
      if (VEC && full) {
        const prdc_f32x4 q = *reinterpret_cast<const prdc_f32x4*>(p);
        v[u][0] = q[0]; v[u][1] = q[1]; v[u][2] = q[2]; v[u][3] = q[3];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[u][j] = c0 + j < cols ? p[j] : inf;
      }
    }
#pragma unroll
    for (int u = 0; u < PD_U; ++u) {
      const int r = rb + u;
      if (r < r1) {                                     // wave-uniform
        const float add = row_add ? row_add[r] : 0.f;
        const float tr = thr_row ? thr_row[r] : -inf;
        float m = inf;
        int h = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = v[u][j] + add;
          m = fminf(m, d);
          h |= d < tc[j] ? 1 : 0;
          cnt[j] += d < tr ? 1 : 0;
        }
        m = prdc_wave_min(m);
        h = __any(h);
        if (lane == 0) {
          smin[wave][r - r0] = m;
          shit[wave][r - r0] = h ? 1 : 0;
        }
      }
    }
  }
  __syncthreads();
  if (tid < r1 - r0) {
    const size_t o = (size_t)blockIdx.x * rows + r0 + tid;
    ws_min[o] = fminf(fminf(smin[0][tid], smin[1][tid]), fminf(smin[2][tid], smin[3][tid]));
    ws_hit[o] = shit[0][tid] | shit[1][tid] | shit[2][tid] | shit[3][tid];
  }
  if (thr_row) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < cols) ws_cnt[(size_t)blockIdx.y * cols + c0 + j] = cnt[j];
  }
}

// Workgroup = 64 outputs x 4 slices of the tile index; blocks [0, nbr) finish rows, [nbr, nbr + nbc) finish columns.
__global__ __launch_bounds__(PD_T) void prdc_finish_kernel(const float* __restrict__ ws_min, const int* __restrict__ ws_hit,
                                                           const int* __restrict__ ws_cnt, int rows, int cols, int nct, int nrt,
                                                           int nbr, float* __restrict__ row_min, int* __restrict__ row_hit,
                                                           int* __restrict__ col_hit, int* __restrict__ col_count,
                                                           int accumulate) {
  __shared__ float sm[4][64];
  __shared__ int si[4][64];
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  if ((int)blockIdx.x < nbr) {
    const long r = (long)blockIdx.x * 64 + lane;
    float m = __builtin_huge_valf();
    int h = 0;
    if (r < rows)
      for (int t = slice; t < nct; t += 4) {
        m = fminf(m, ws_min[(size_t)t * rows + r]);
        h |= ws_hit[(size_t)t * rows + r];
      }
    sm[slice][lane] = m;
    si[slice][lane] = h;
    __syncthreads();
    if (slice == 0 && r < rows) {
      row_min[r] = fminf(fminf(sm[0][lane], sm[1][lane]), fminf(sm[2][lane], sm[3][lane]));
      row_hit[r] = si[0][lane] | si[1][lane] | si[2][lane] | si[3][lane];
    }
  } else {
    const long c = (long)(blockIdx.x - nbr) * 64 + lane;
    int s = 0;
    if (c < cols)
      for (int t = slice; t < nrt; t += 4) s += ws_cnt[(size_t)t * cols + c];
    si[slice][lane] = s;
    __syncthreads();
    if (slice == 0 && c < cols) {
      s = (si[0][lane] + si[1][lane]) + (si[2][lane] + si[3][lane]);
      const int hit = s > 0 ? 1 : 0;
      col_count[c] = accumulate ? col_count[c] + s : s;
      col_hit[c] = accumulate ? (col_hit[c] | hit) : hit;
    }
  }
}

static bool prdc_shape_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && cdiv(rows, PD_TR) <= 65535; }

}  // namespace diagan

using namespace diagan;

DIAGAN_API size_t diagan_prdc_reduce_ws(int rows, int cols) {
  if (!prdc_shape_ok(rows, cols)) return 0;
  const size_t nct = cdiv(cols, PD_TC), nrt = cdiv(rows, PD_TR);
  return (2 * nct * (size_t)rows + nrt * (size_t)cols) * 4;
}

DIAGAN_API int diagan_prdc_reduce(const float* T, const float* row_add, const float* thr_col, const float* thr_row, int rows,
                                  int cols, int ld, float* row_min, int* row_hit, int* col_hit, int* col_count, int accumulate,
                                  void* ws, int64_t ws_bytes, void* stream) {
  DG_REQUIRE(prdc_shape_ok(rows, cols) && ld >= cols, "prdc_reduce: bad shape rows=%d cols=%d ld=%d", rows, cols, ld);
  DG_REQUIRE(T && thr_col && row_min && row_hit, "prdc_reduce: null pointer (T, thr_col, row_min, row_hit are required)");
  DG_REQUIRE(!thr_row || (col_hit && col_count), "prdc_reduce: thr_row given without col_hit / col_count");
  const size_t need = diagan_prdc_reduce_ws(rows, cols);
  DG_REQUIRE(ws && ws_bytes >= 0 && (size_t)ws_bytes >= need && ((uintptr_t)ws & 15) == 0,
             "prdc_reduce: workspace of %ld bytes, %zu needed (16-byte aligned)", (long)ws_bytes, need);
  const int nct = cdiv(cols, PD_TC), nrt = cdiv(rows, PD_TR);
  float* ws_min = (float*)ws;
  int* ws_hit = (int*)ws + (size_t)nct * rows;
  int* ws_cnt = ws_hit + (size_t)nct * rows;
  const bool vec = ((uintptr_t)T & 15) == 0 && (ld & 3) == 0;
  const dim3 grid(nct, nrt);
  if (vec)
    hipLaunchKernelGGL(prdc_tile_kernel<true>, grid, dim3(PD_T), 0, (hipStream_t)stream, T, row_add, thr_col, thr_row, rows, cols,
                       (long)ld, ws_min, ws_hit, ws_cnt);
  else
    hipLaunchKernelGGL(prdc_tile_kernel<false>, grid, dim3(PD_T), 0, (hipStream_t)stream, T, row_add, thr_col, thr_row, rows,
                       cols, (long)ld, ws_min, ws_hit, ws_cnt);
  int rc = check_launch("prdc_reduce (tiles)");
  if (rc) return rc;
  const int nbr = cdiv(rows, 64), nbc = thr_row ? cdiv(cols, 64) : 0;
  hipLaunchKernelGGL(prdc_finish_kernel, dim3(nbr + nbc), dim3(PD_T), 0, (hipStream_t)stream, ws_min, ws_hit, ws_cnt, rows, cols,
                     nct, nrt, nbr, row_min, row_hit, col_hit, col_count, accumulate);
  return check_launch("prdc_reduce (finish)");
}
