// The pictures: a batch of fp32 images tiled into one uint8 HWC grid, byte for byte what torchvision 0.8.2's
// make_grid + save_image give on torch CPU fp32 (include/diagan_pictures.h states the contract).
//
//   pic_minmax_*      min and max of an fp32 array: partial extremes per workgroup into the caller's workspace, then one workgroup
//                     combines them.  Minimum and maximum do not depend on the order, so neither does the result.
//   pic_grid_kernel   output-driven: a lane owns four consecutive pixels of one grid row, finds for each the image and the place it
//                     comes from (or that it is padding), reads the C planes there, normalises, converts and stores 12 bytes --
//                     three 4-byte stores when Wg % 4 == 0 (every run then starts at a multiple of 12 bytes), bytes otherwise.
//                     Neighbouring lanes read neighbouring floats of the same image row.
//
// The arithmetic is the reference's, operation by operation: this file is compiled with -ffp-contract=off (v * 255 + 0.5 as one
// fma changes bytes), the divisor of norm_ip is formed in double and rounded to fp32 once, and `/` on floats is hipcc's correctly
// rounded division (-fhip-fp32-correctly-rounded-divide-sqrt, its default, restated in the Makefile).
#include "common.h"
#include "diagan_pictures.h"

#include <algorithm>

namespace diagan {

constexpr int PIC_T = 256;
constexpr int PIC_MAX_BLOCKS = 2048;      // memory-bound: cap the grid and stride the rest
constexpr int PIC_MM_BLOCKS = 1024;       // partial extremes of diagan_pic_minmax, at most
constexpr int PIC_MM_PER_LANE = 8;        // elements a lane reads before another workgroup is worth starting

static int pic_minmax_blocks(int64_t n) {
  const int64_t per_block = (int64_t)PIC_T * PIC_MM_PER_LANE;
  return (int)std::min<int64_t>(PIC_MM_BLOCKS, (n + per_block - 1) / per_block);
}

__device__ __forceinline__ void pic_block_minmax(float lo, float hi, float* __restrict__ out) {
  __shared__ float slo[PIC_T / 64], shi[PIC_T / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    slo[threadIdx.x >> 6] = lo;
    shi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < PIC_T / 64; ++w) {
      lo = fminf(lo, slo[w]);
      hi = fmaxf(hi, shi[w]);
    }
    out[0] = lo;
    out[1] = hi;
  }
}

// every lane starts from x[0], a member of the set, so lanes without elements of their own change nothing
__global__ __launch_bounds__(PIC_T) void pic_minmax_partial_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ part) {
  float lo = x[0], hi = lo;
  for (int64_t i = (int64_t)blockIdx.x * PIC_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PIC_T) {
    const float v = x[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  pic_block_minmax(lo, hi, part + 2 * blockIdx.x);
}

__global__ __launch_bounds__(PIC_T) void pic_minmax_final_kernel(const float* __restrict__ part, int blocks, float* __restrict__ lohi) {
  float lo = part[0], hi = part[1];
  for (int b = threadIdx.x; b < blocks; b += PIC_T) {
    lo = fminf(lo, part[2 * b]);
    hi = fmaxf(hi, part[2 * b + 1]);
  }
  pic_block_minmax(lo, hi, lohi);
}

struct PicGrid {
  int B, C, H, W, xmaps, ymaps, padding, Hg, Wg;
  float pad_value;
  int norm, passes, bytes;
  double lo, hi;
};

// what norm_ip applies, in the types torch CPU applies it in: clamp bounds and the addend as fp32, the divisor from doubles
struct PicNorm {
  float lo, hi, neg_lo, div;
  float hi2, div2;                        // second pass: lo2 = 0
};

__device__ __forceinline__ PicNorm pic_norm(const PicGrid& g, const float* __restrict__ lohi) {
  PicNorm n;
  const double lo = g.norm == DIAGAN_PIC_NORM_DATA ? (double)lohi[0] : g.lo;
  const double hi = g.norm == DIAGAN_PIC_NORM_DATA ? (double)lohi[1] : g.hi;
  n.lo = (float)lo;
  n.hi = (float)hi;
  n.neg_lo = (float)(-lo);
  n.div = (float)(hi - lo + 1e-5);
  // the image of the data maximum under the first pass is the maximum of the grid, its minimum is 0 (the data minimum, and the
  // padding of 0)
  n.hi2 = (fminf(fmaxf(n.hi, n.lo), n.hi) + n.neg_lo) / n.div;
  n.div2 = (float)((double)n.hi2 - 0.0 + 1e-5);
  return n;
}

__device__ __forceinline__ uint32_t pic_byte(float v, int bytes) {
  if (bytes == DIAGAN_PIC_BYTES_TO_NUMPY) {
    v = (v + 1.0f) / 2.0f;
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    v = v * 255.0f;
  } else {
    v = v * 255.0f;
    v = v + 0.5f;
    v = fminf(fmaxf(v, 0.0f), 255.0f);
  }
  return (uint32_t)(int)v;                // in [0, 255]: truncation
}

// item = (grid row y, run r of four pixels): x0 = 4 r.  WORDS: the run is whole and 4-byte aligned (Wg % 4 == 0)
template <bool WORDS>
__global__ __launch_bounds__(PIC_T) void pic_grid_kernel(const float* __restrict__ x, PicGrid g, const float* __restrict__ lohi,
                                                         uint8_t* __restrict__ out) {
  PicNorm nm = {};
  if (g.norm != DIAGAN_PIC_NORM_NONE) nm = pic_norm(g, lohi);
  const uint32_t pad_byte = pic_byte(g.pad_value, g.bytes);
  const int runs = (g.Wg + 3) >> 2;
  const int cell_h = g.H + g.padding, cell_w = g.W + g.padding;
  const int64_t plane = (int64_t)g.H * g.W;
  const int64_t items = (int64_t)g.Hg * runs;
  for (int64_t i = (int64_t)blockIdx.x * PIC_T + threadIdx.x; i < items; i += (int64_t)gridDim.x * PIC_T) {
    const int y = (int)(i / runs), x0 = 4 * (int)(i - (int64_t)y * runs);
    int cy = 0, iy = y;                   // B == 1: the grid is the image
    if (g.B > 1) {
      cy = y / cell_h;
      iy = y - cy * cell_h - g.padding;
    }
    const bool row_in = iy >= 0 && cy < g.ymaps;
    uint32_t px[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xx = x0 + k;
      int cx = 0, ix = xx;
      if (g.B > 1) {
        cx = xx / cell_w;
        ix = xx - cx * cell_w - g.padding;
      }
      const int img = cy * g.xmaps + cx;
      const bool in = row_in && xx < g.Wg && ix >= 0 && cx < g.xmaps && img < g.B;
      uint32_t b[3] = {pad_byte, pad_byte, pad_byte};
      if (in) {
        const float* p = x + ((int64_t)img * g.C * g.H + iy) * g.W + ix;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (c < g.C) {
            float v = p[c * plane];
            if (g.norm != DIAGAN_PIC_NORM_NONE) {
              v = fminf(fmaxf(v, nm.lo), nm.hi);
              v = (v + nm.neg_lo) / nm.div;
              if (g.passes == 2) {
                v = fminf(fmaxf(v, 0.0f), nm.hi2);
                v = v / nm.div2;          // + (-0.0f) changes nothing
              }
            }
            b[c] = pic_byte(v, g.bytes);
          } else {
            b[c] = b[0];
          }
        }
      }
      px[3 * k] = b[0];
      px[3 * k + 1] = b[1];
      px[3 * k + 2] = b[2];
    }
    uint8_t* o = out + ((int64_t)y * g.Wg + x0) * 3;
    if (WORDS) {
      uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
      for (int j = 0; j < 3; ++j)
        o4[j] = px[4 * j] | (px[4 * j + 1] << 8) | (px[4 * j + 2] << 16) | (px[4 * j + 3] << 24);
    } else {
      const int nb = 3 * min(4, g.Wg - x0);
#pragma unroll
      for (int j = 0; j < 12; ++j)
        if (j < nb) o[j] = (uint8_t)px[j];
    }
  }
}

static int pic_shape(const char* who, int B, int H, int W, int nrow, int padding, PicGrid* g) {
  DG_REQUIRE(B >= 1, "%s: B=%d", who, B);
  DG_REQUIRE(H >= 1 && W >= 1, "%s: bad image size H=%d W=%d", who, H, W);
  DG_REQUIRE(nrow >= 1, "%s: nrow=%d", who, nrow);
  DG_REQUIRE(padding >= 0, "%s: padding=%d", who, padding);
  const int xmaps = std::min(nrow, B), ymaps = (B + xmaps - 1) / xmaps;
  int64_t Hg = (int64_t)ymaps * ((int64_t)H + padding) + padding, Wg = (int64_t)xmaps * ((int64_t)W + padding) + padding;
  if (B == 1) Hg = H, Wg = W;
  DG_REQUIRE(Hg < (1LL << 31) && Wg < (1LL << 31) && (int64_t)H + padding < (1LL << 31) && (int64_t)W + padding < (1LL << 31),
             "%s: a grid of %ld x %ld exceeds 2^31 in one dimension", who, (long)Hg, (long)Wg);
  g->B = B, g->H = H, g->W = W, g->xmaps = xmaps, g->ymaps = ymaps, g->padding = padding, g->Hg = (int)Hg, g->Wg = (int)Wg;
  return DIAGAN_OK;
}

}  // namespace diagan

using namespace diagan;

DIAGAN_API size_t diagan_pic_minmax_ws(int64_t n) { return n < 1 ? 0 : (size_t)pic_minmax_blocks(n) * 2 * sizeof(float); }

DIAGAN_API int diagan_pic_minmax(const float* x, int64_t n, float* lohi, void* ws, int64_t ws_bytes, void* stream) {
  DG_REQUIRE(x != nullptr && lohi != nullptr && ws != nullptr, "diagan_pic_minmax: null pointer");
  DG_REQUIRE(n >= 1, "diagan_pic_minmax: n=%ld", (long)n);
  DG_REQUIRE(ws_bytes >= (int64_t)diagan_pic_minmax_ws(n) && ((uintptr_t)ws & 3) == 0,
             "diagan_pic_minmax: workspace of %ld bytes, %ld needed (4-byte aligned)", (long)ws_bytes, (long)diagan_pic_minmax_ws(n));
  hipStream_t s = (hipStream_t)stream;
  const int blocks = pic_minmax_blocks(n);
  float* part = (float*)ws;
  hipLaunchKernelGGL(pic_minmax_partial_kernel, dim3(blocks), dim3(PIC_T), 0, s, x, n, part);
  hipLaunchKernelGGL(pic_minmax_final_kernel, dim3(1), dim3(PIC_T), 0, s, (const float*)part, blocks, lohi);
  return check_launch("diagan_pic_minmax");
}

DIAGAN_API int diagan_pic_grid_shape(int B, int H, int W, int nrow, int padding, int* hw_host) {
  DG_REQUIRE(hw_host != nullptr, "diagan_pic_grid_shape: null pointer");
  PicGrid g = {};
  const int rc = pic_shape("diagan_pic_grid_shape", B, H, W, nrow, padding, &g);
  if (rc != DIAGAN_OK) return rc;
  hw_host[0] = g.Hg;
  hw_host[1] = g.Wg;
  return DIAGAN_OK;
}

DIAGAN_API int diagan_pic_grid(const float* x, int B, int C, int H, int W, int nrow, int padding, float pad_value, int norm, double lo,
                               double hi, const float* lohi, int passes, int bytes, void* out, void* stream) {
  DG_REQUIRE(x != nullptr && out != nullptr && (norm != DIAGAN_PIC_NORM_DATA || lohi != nullptr), "diagan_pic_grid: null pointer");
  DG_REQUIRE(B >= 1, "diagan_pic_grid: B=%d", B);
  DG_REQUIRE(C == 1 || C == 3, "diagan_pic_grid: C=%d is neither 1 nor 3", C);
  PicGrid g = {};
  const int rc = pic_shape("diagan_pic_grid", B, H, W, nrow, padding, &g);
  if (rc != DIAGAN_OK) return rc;
  DG_REQUIRE(norm == DIAGAN_PIC_NORM_NONE || norm == DIAGAN_PIC_NORM_RANGE || norm == DIAGAN_PIC_NORM_DATA,
             "diagan_pic_grid: norm=%d", norm);
  DG_REQUIRE(passes == 1 || passes == 2, "diagan_pic_grid: passes=%d", passes);
  DG_REQUIRE(bytes == DIAGAN_PIC_BYTES_SAVE_IMAGE || bytes == DIAGAN_PIC_BYTES_TO_NUMPY, "diagan_pic_grid: bytes=%d", bytes);
  if (passes == 2 && !(norm == DIAGAN_PIC_NORM_DATA && pad_value == 0.0f))
    return set_err(DIAGAN_EUNSUP, "diagan_pic_grid: two passes need the device range (norm=%d) and pad_value == 0, got norm=%d "
                   "pad_value=%g", DIAGAN_PIC_NORM_DATA, norm, (double)pad_value);
  g.C = C, g.pad_value = pad_value, g.norm = norm, g.passes = passes, g.bytes = bytes, g.lo = lo, g.hi = hi;
  hipStream_t s = (hipStream_t)stream;
  const int64_t items = (int64_t)g.Hg * ((g.Wg + 3) / 4);
  const int blocks = (int)std::min<int64_t>(PIC_MAX_BLOCKS, (items + PIC_T - 1) / PIC_T);
  if (g.Wg % 4 == 0 && ((uintptr_t)out & 3) == 0)
    hipLaunchKernelGGL(pic_grid_kernel<true>, dim3(blocks), dim3(PIC_T), 0, s, x, g, lohi, (uint8_t*)out);
  else
    hipLaunchKernelGGL(pic_grid_kernel<false>, dim3(blocks), dim3(PIC_T), 0, s, x, g, lohi, (uint8_t*)out);
  return check_launch("diagan_pic_grid");
}
