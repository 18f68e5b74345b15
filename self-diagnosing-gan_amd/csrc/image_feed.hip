// The image feed of the StyleGAN2 trainers: the two kernels the packed uint8 sets need beyond data_feed.hip.
//
//   img_fetch_flip_*          the hot path: data_fetch_* with the one random step of the reference's transform
//                             (RandomHorizontalFlip, train_ffhq.py:590) folded into the gather.  flip[b] mirrors item b along x;
//                             the values are those of kFetchTable, the table of data_feed.hip, read through its device address
//                             and copied to LDS by each workgroup.  Same store-side layout as data_fetch_quad_kernel: a lane
//                             owns four consecutive output pixels and issues one 16-byte store into each of the C planes.  When
//                             W % 4 == 0 the four pixels of a mirrored quad are the mirrored quad of the same row in reverse
//                             order, still 4 C contiguous bytes; a mirrored item whose W is no multiple of four (the quad then
//                             spans rows) gathers its bytes one by one.  Planes that are no multiple of four floats take the
//                             scalar kernel.
//   img_resize_crop_banded    ingest: data_resize_crop_kernel with the LDS intermediate cut into bands of output rows, so that a
//                             1024 x 1024 source fits, and with coefficients that may be negative (Lanczos).  One workgroup per
//                             (image, band): it finds the source rows its band reads from vb, writes their horizontal pass to
//                             LDS, then runs the vertical pass.  Rows between two bands are computed by both.  Not written for
//                             speed: decode dominates ingest.
//
// int32 is enough for the sums.  With k the coefficients of one output position, P the sum of its positive and M the sum of the
// magnitudes of its negative ones, every partial sum of 2^21 + sum pix * k with pix in [0, 255] lies in
// [-255 M, 2^21 + 255 P].  Unnormalised tables do not fit (25 taps of 2^22 give 25 * 255 * 2^22 = 2.7e10), so the header makes
// P <= 2^23 the precondition: 2^21 + 255 * 2^23 = 2 141 192 192 < 2^31 - 1.  PIL's tables are normalised, P - M = 2^22 up to the
// rounding of each tap (at most taps / 2), so the condition is M <= 2^22: negative lobes that weigh less than the whole filter.
// Lanczos-3 has M / 2^22 of about 0.16 (the host plan, diagan/datasets/transform.py, asserts the bound on every table it makes).
#include "common.h"
#include "data_feed.h"
#include "diagan_images.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace diagan {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int IF_T = 256;
constexpr int IF_MAX_BLOCKS = 2048;       // memory-bound: cap the grid and stride the rest
constexpr int64_t IF_LDS_LIMIT = 160 * 1024;
constexpr int IF_LDS_HEAD = 16;           // the band's source row range, ahead of the intermediate rows

// HW % 4 == 0: item = (batch row b, quad q of four consecutive output pixels); C in {1, 3}
template <int C>
__global__ __launch_bounds__(IF_T) void img_fetch_flip_quad_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                                   int64_t lo, const uint8_t* __restrict__ flip, int B, int H,
                                                                   int W, const float* __restrict__ table,
                                                                   float* __restrict__ dst) {
  __shared__ float lut[256];
  lut[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const int HW = H * W, Q = HW >> 2;
  const bool rows_of_quads = (W & 3) == 0;
  const int64_t items = (int64_t)B * Q;
  for (int64_t i = (int64_t)blockIdx.x * IF_T + threadIdx.x; i < items; i += (int64_t)gridDim.x * IF_T) {
    const int b = (int)(i / Q), q = (int)(i - (int64_t)b * Q);
    const int64_t row = idx != nullptr ? idx[b] : lo + b;
    const bool f = flip != nullptr && flip[b] != 0;
    const uint8_t* img = src + row * ((int64_t)HW * C);
    uint8_t px[4 * C];                                      // pixel k, channel c at k * C + c, in OUTPUT order
    if (!f || rows_of_quads) {
      // 4 C bytes at a 4-byte aligned address: the row stride HW * C and the quad offset 4 C q are multiples of 4.  Mirrored:
      // the quad at the mirrored place of the same image row, its pixels taken last to first
      int sq = q;
      if (f) {
        const int qw = W >> 2, y = q / qw;
        sq = y * qw + (qw - 1 - (q - y * qw));
      }
      const uint32_t* p = reinterpret_cast<const uint32_t*>(img + (int64_t)sq * (4 * C));
      uint32_t w[C];
#pragma unroll
      for (int j = 0; j < C; ++j) w[j] = p[j];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int straight = k * C + c, mirrored = (3 - k) * C + c;
          const uint32_t a = (w[straight >> 2] >> (8 * (straight & 3))) & 255u;
          const uint32_t m = (w[mirrored >> 2] >> (8 * (mirrored & 3))) & 255u;
          px[k * C + c] = (uint8_t)(f ? m : a);
        }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = 4 * q + k, y = p / W, x = p - y * W;
        const uint8_t* s = img + (int64_t)(y * W + (W - 1 - x)) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) px[k * C + c] = s[c];
      }
    }
    float* out = dst + (int64_t)b * C * HW + 4 * q;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = lut[px[k * C + c]];
      *reinterpret_cast<f32x4*>(out + (int64_t)c * HW) = o;
    }
  }
}

// any H, W, C: one lane per output element, stores coalesced along a plane
__global__ __launch_bounds__(IF_T) void img_fetch_flip_scalar_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                                     int64_t lo, const uint8_t* __restrict__ flip, int B, int H,
                                                                     int W, int C, const float* __restrict__ table,
                                                                     float* __restrict__ dst) {
  __shared__ float lut[256];
  lut[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const int HW = H * W;
  const int64_t per = (int64_t)C * HW, total = (int64_t)B * per;
  for (int64_t e = (int64_t)blockIdx.x * IF_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * IF_T) {
    const int b = (int)(e / per);
    const int r = (int)(e - (int64_t)b * per);
    const int c = r / HW, p = r - c * HW;
    const int y = p / W, x = p - y * W;
    const int64_t row = idx != nullptr ? idx[b] : lo + b;
    const int sx = (flip != nullptr && flip[b] != 0) ? W - 1 - x : x;
    dst[e] = lut[src[row * per + (int64_t)(y * W + sx) * C + c]];
  }
}

__device__ __forceinline__ int img_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one workgroup per (image, band of band_rows output rows): blockIdx.x = image * bands + band.  Tables as in
// data_resize_crop_kernel.  lds = [r0, r1 of the band | horizontal pass of source rows [r0, r1): [r1 - r0][Wo][C]]
__global__ __launch_bounds__(IF_T) void img_resize_crop_banded_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int C,
                                                                      uint8_t* __restrict__ dst, int Ho, int Wo,
                                                                      const int* __restrict__ hb, const int* __restrict__ hk,
                                                                      int hks, const int* __restrict__ vb,
                                                                      const int* __restrict__ vk, int vks, int band_rows,
                                                                      int bands, int lds_rows) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  int* range = reinterpret_cast<int*>(lds);
  uint8_t* tmp = lds + IF_LDS_HEAD;
  const int image = blockIdx.x / bands, band = blockIdx.x - image * bands;
  const int y0 = band * band_rows, y1 = min(Ho, y0 + band_rows);
  if (threadIdx.x == 0) {
    range[0] = INT_MAX;
    range[1] = 0;
  }
  __syncthreads();
  int first = INT_MAX, last = 0;
  for (int y = y0 + threadIdx.x; y < y1; y += IF_T) {
    first = min(first, vb[2 * y]);
    last = max(last, vb[2 * y] + vb[2 * y + 1]);
  }
  if (first < last) {
    atomicMin(&range[0], first);
    atomicMax(&range[1], last);
  }
  __syncthreads();
  const int r0 = range[0], r1 = range[1];
  // the host sized the LDS from the same table and checked it against [0, Hs): this only holds if vb changed in between
  if (r0 < 0 || r1 > Hs || r1 - r0 > lds_rows) return;

  const uint8_t* in = src + (int64_t)image * Hs * Ws * C;
  uint8_t* out = dst + (int64_t)image * Ho * Wo * C;
  const int WoC = Wo * C;
  const int n1 = (r1 - r0) * WoC;
  for (int e = threadIdx.x; e < n1; e += IF_T) {
    const int r = e / WoC, xc = e - r * WoC;
    const int x = xc / C, c = xc - x * C;
    const int x0 = hb[2 * x], cnt = hb[2 * x + 1];
    const uint8_t* line = in + ((int64_t)(r0 + r) * Ws + x0) * C + c;
    const int* k = hk + (int64_t)x * hks;
    int ss = 1 << 21;
    for (int j = 0; j < cnt; ++j) ss += (int)line[j * C] * k[j];
    tmp[e] = (uint8_t)img_clip8(ss >> 22);                  // >> of a negative sum is arithmetic, as in PIL's C
  }
  __syncthreads();
  const int n2 = (y1 - y0) * WoC;
  for (int e = threadIdx.x; e < n2; e += IF_T) {
    const int yy = e / WoC, xc = e - yy * WoC;
    const int y = y0 + yy;
    const int f0 = vb[2 * y], cnt = vb[2 * y + 1];
    const uint8_t* col = tmp + (f0 - r0) * WoC + xc;
    const int* k = vk + (int64_t)y * vks;
    int ss = 1 << 21;
    for (int j = 0; j < cnt; ++j) ss += (int)col[j * WoC] * k[j];
    out[(int64_t)y * WoC + xc] = (uint8_t)img_clip8(ss >> 22);
  }
}

static FuncAttrLatch g_banded_lds;

}  // namespace diagan

using namespace diagan;

DIAGAN_API int diagan_img_fetch_flip(const void* src, int64_t N, int H, int W, int C, const int64_t* idx, int64_t lo,
                                     const void* flip, int B, float* dst, void* stream) {
  DG_REQUIRE(src != nullptr && dst != nullptr, "diagan_img_fetch_flip: null pointer");
  DG_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && B >= 0, "diagan_img_fetch_flip: bad shape N=%ld H=%d W=%d C=%d B=%d", (long)N, H, W,
             C, B);
  DG_REQUIRE((int64_t)H * W * C < (1LL << 31), "diagan_img_fetch_flip: one image of %d x %d x %d exceeds 2^31 bytes", H, W, C);
  DG_REQUIRE(idx != nullptr || (lo >= 0 && lo + B <= N), "diagan_img_fetch_flip: range [%ld, %ld) outside [0, %ld)", (long)lo,
             (long)(lo + B), (long)N);
  if (B == 0) return DIAGAN_OK;
  hipStream_t s = (hipStream_t)stream;
  const float* table = nullptr;
  DG_HIP(fetch_table_device(&table));
  const int HW = H * W;
  const uint8_t* in = (const uint8_t*)src;
  const uint8_t* fl = (const uint8_t*)flip;
  const bool aligned = ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 15) == 0;      // 4-byte loads, 16-byte stores
  if (HW % 4 == 0 && (C == 1 || C == 3) && aligned) {
    const int blocks = (int)std::min<int64_t>(IF_MAX_BLOCKS, ((int64_t)B * (HW / 4) + IF_T - 1) / IF_T);
    if (C == 1)
      hipLaunchKernelGGL(img_fetch_flip_quad_kernel<1>, dim3(blocks), dim3(IF_T), 0, s, in, idx, lo, fl, B, H, W, table, dst);
    else
      hipLaunchKernelGGL(img_fetch_flip_quad_kernel<3>, dim3(blocks), dim3(IF_T), 0, s, in, idx, lo, fl, B, H, W, table, dst);
  } else {
    const int blocks = (int)std::min<int64_t>(IF_MAX_BLOCKS, ((int64_t)B * C * HW + IF_T - 1) / IF_T);
    hipLaunchKernelGGL(img_fetch_flip_scalar_kernel, dim3(blocks), dim3(IF_T), 0, s, in, idx, lo, fl, B, H, W, C, table, dst);
  }
  return check_launch("diagan_img_fetch_flip");
}

DIAGAN_API int diagan_img_resize_crop_banded(const void* src, int n, int Hs, int Ws, int C, void* dst, int Ho, int Wo, const int* hb,
                                             const int* hk, int hks, const int* vb, const int* vk, int vks, int band_rows,
                                             void* stream) {
  DG_REQUIRE(src != nullptr && dst != nullptr && hb != nullptr && hk != nullptr && vb != nullptr && vk != nullptr,
             "diagan_img_resize_crop_banded: null pointer");
  DG_REQUIRE(n >= 0 && Hs > 0 && Ws > 0 && C > 0 && Ho > 0 && Wo > 0 && hks > 0 && vks > 0,
             "diagan_img_resize_crop_banded: bad shape n=%d %dx%dx%d -> %dx%d", n, Hs, Ws, C, Ho, Wo);
  DG_REQUIRE(band_rows > 0, "diagan_img_resize_crop_banded: band_rows=%d", band_rows);
  DG_REQUIRE((int64_t)Hs * Ws * C < (1LL << 31) && (int64_t)Ho * Wo * C < (1LL << 31),
             "diagan_img_resize_crop_banded: image too large");
  band_rows = std::min(band_rows, Ho);
  const int bands = (Ho + band_rows - 1) / band_rows;
  DG_REQUIRE((int64_t)n * bands < (1LL << 31), "diagan_img_resize_crop_banded: %d images x %d bands exceed the grid", n, bands);
  hipStream_t s = (hipStream_t)stream;
  // the vertical bounds, read back: they size the LDS and are the only indices into it
  std::vector<int> rows((size_t)Ho * 2);
  DG_HIP(hipMemcpyAsync(rows.data(), vb, rows.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  DG_HIP(hipStreamSynchronize(s));
  int span = 0;
  for (int y0 = 0; y0 < Ho; y0 += band_rows) {
    int first = INT_MAX, last = 0;
    for (int y = y0; y < std::min(Ho, y0 + band_rows); ++y) {
      const int f = rows[2 * y], t = rows[2 * y + 1];
      DG_REQUIRE(f >= 0 && t >= 1 && t <= vks && f <= Hs - t,
                 "diagan_img_resize_crop_banded: output row %d reads source rows [%d, %d + %d) with Hs=%d, vks=%d", y, f, f, t, Hs, vks);
      first = std::min(first, f);
      last = std::max(last, f + t);
    }
    span = std::max(span, last - first);
  }
  const int64_t lds = IF_LDS_HEAD + (int64_t)span * Wo * C;
  if (lds > IF_LDS_LIMIT)
    return set_err(DIAGAN_EUNSUP,
                   "diagan_img_resize_crop_banded: a band of %d output rows reads %d source rows, %ld bytes of intermediate rows "
                   "exceed the 160 KiB of LDS", band_rows, span, (long)lds);
  if (n == 0) return DIAGAN_OK;
  DG_LDS(g_banded_lds, img_resize_crop_banded_kernel, (size_t)lds);
  hipLaunchKernelGGL(img_resize_crop_banded_kernel, dim3(n * bands), dim3(IF_T), (size_t)lds, s, (const uint8_t*)src, Hs, Ws, C,
                     (uint8_t*)dst, Ho, Wo, hb, hk, hks, vb, vk, vks, band_rows, bands, span);
  return check_launch("diagan_img_resize_crop_banded");
}
