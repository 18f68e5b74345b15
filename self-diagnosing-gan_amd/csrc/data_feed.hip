// Device-resident datasets: the images stay in HBM as uint8 NHWC at the training size, and two kernels touch them.
//
//   data_fetch_*        the hot path: rows of src [N,H,W,C] uint8, picked by a device int64 index vector (any order, repeats) or
//                       as the range [lo, lo+B), become the fp32 NCHW batch [B,C,H,W] that train_step and netD(x) take.  Every
//                       value is ToTensor + Normalize(0.5, 0.5) of the reference's transforms (diagan-pkg/diagan/datasets/
//                       transform.py:9-10), (v / 255 - 0.5) / 0.5 in fp32 with every step rounded as the torch CPU sequence
//                       t.float().div(255).sub(0.5).div(0.5) rounds it: the 256 possible results are a table evaluated by the
//                       compiler in IEEE arithmetic (kFetchTable), copied to LDS by each workgroup.
//                       Written for the store side (a 64 x 3 x 32 x 32 batch reads 196 KB and writes 786 KB): a lane owns four
//                       consecutive pixels, loads their 4 C contiguous bytes and issues one 16-byte store into each of the C
//                       planes, so a wave writes 1 KiB contiguously per plane and reads 256 C contiguous bytes.  Planes whose
//                       size is no multiple of four floats take the scalar kernel (one lane per output element).
//   data_resize_crop    ingest, once per dataset: Resize(s) + CenterCrop(s) of the same transforms, bit-identical to PIL's 8-bit
//                       bilinear path -- a horizontal pass, a rounded uint8 intermediate, a vertical pass, each
//                       clip8((2^21 + sum pix * k) >> 22) with integer coefficients.  The coefficient tables are made on the host
//                       in float64 (diagan/datasets/transform.py) for the output columns and rows that survive the crop; the
//                       kernel does integer arithmetic only.  One workgroup per image, the horizontal-pass intermediate (only the
//                       source rows the kept output rows read) in LDS.  Not written for speed: JPEG decode dominates ingest.
//
// In-range indices and in-range tables are preconditions the Python wrappers establish on the host (diagan/datasets/device.py).
// No allocation, no synchronisation; everything runs on the caller's stream.
#include "common.h"
#include "data_feed.h"
#include "diagan_data.h"

#include <algorithm>

namespace diagan {

struct FetchTable {
  float v[256];
};
constexpr FetchTable make_fetch_table() {
  FetchTable t{};
  for (int i = 0; i < 256; ++i) t.v[i] = ((float)i / 255.0f - 0.5f) / 0.5f;
  return t;
}
constexpr FetchTable kFetchTableHost = make_fetch_table();
__constant__ FetchTable kFetchTable = make_fetch_table();

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DF_T = 256;
constexpr int DF_MAX_BLOCKS = 2048;       // memory-bound: cap the grid and stride the rest

// HW % 4 == 0: item = (batch row b, quad q of four consecutive pixels); C in {1, 3}
template <int C>
__global__ __launch_bounds__(DF_T) void data_fetch_quad_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                               int64_t lo, int B, int HW, float* __restrict__ dst) {
  __shared__ float lut[256];
  lut[threadIdx.x] = kFetchTable.v[threadIdx.x];
  __syncthreads();
  const int Q = HW >> 2;
  const int64_t items = (int64_t)B * Q;
  for (int64_t i = (int64_t)blockIdx.x * DF_T + threadIdx.x; i < items; i += (int64_t)gridDim.x * DF_T) {
    const int b = (int)(i / Q), q = (int)(i - (int64_t)b * Q);
    const int64_t row = idx != nullptr ? idx[b] : lo + b;
    // 4 C bytes at a 4-byte aligned address: the row stride HW * C and the quad offset 4 C q are multiples of 4
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src + row * ((int64_t)HW * C) + (int64_t)q * (4 * C));
    uint32_t w[C];
#pragma unroll
    for (int j = 0; j < C; ++j) w[j] = p[j];
    float* out = dst + (int64_t)b * C * HW + 4 * q;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int byte = k * C + c;                       // pixel k, channel c of the 4 C bytes
        o[k] = lut[(w[byte >> 2] >> (8 * (byte & 3))) & 255u];
      }
      *reinterpret_cast<f32x4*>(out + (int64_t)c * HW) = o;
    }
  }
}

// any H, W, C: one lane per output element, stores coalesced along a plane
__global__ __launch_bounds__(DF_T) void data_fetch_scalar_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                                 int64_t lo, int B, int HW, int C, float* __restrict__ dst) {
  __shared__ float lut[256];
  lut[threadIdx.x] = kFetchTable.v[threadIdx.x];
  __syncthreads();
  const int64_t per = (int64_t)C * HW, total = (int64_t)B * per;
  for (int64_t e = (int64_t)blockIdx.x * DF_T + threadIdx.x; e < total; e += (int64_t)gridDim.x * DF_T) {
    const int b = (int)(e / per);
    const int r = (int)(e - (int64_t)b * per);
    const int c = r / HW, p = r - c * HW;
    const int64_t row = idx != nullptr ? idx[b] : lo + b;
    dst[e] = lut[src[row * per + (int64_t)p * C + c]];
  }
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one workgroup per image.  Tables: bounds [out][2] = (first source index, tap count), coefficients [out][ks], for the kept
// output columns (h*) and rows (v*).  tmp holds the horizontal pass of source rows [r0, r1).
__global__ __launch_bounds__(DF_T) void data_resize_crop_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int C,
                                                                uint8_t* __restrict__ dst, int Ho, int Wo,
                                                                const int* __restrict__ hb, const int* __restrict__ hk, int hks,
                                                                const int* __restrict__ vb, const int* __restrict__ vk, int vks,
                                                                int r0, int r1) {
  extern __shared__ uint8_t tmp[];        // [r1 - r0][Wo][C]
  const uint8_t* in = src + (int64_t)blockIdx.x * Hs * Ws * C;
  uint8_t* out = dst + (int64_t)blockIdx.x * Ho * Wo * C;
  const int WoC = Wo * C;
  const int n1 = (r1 - r0) * WoC;
  for (int e = threadIdx.x; e < n1; e += DF_T) {
    const int r = e / WoC, xc = e - r * WoC;
    const int x = xc / C, c = xc - x * C;
    const int x0 = hb[2 * x], cnt = hb[2 * x + 1];
    const uint8_t* line = in + ((int64_t)(r0 + r) * Ws + x0) * C + c;
    const int* k = hk + (int64_t)x * hks;
    int ss = 1 << 21;
    for (int j = 0; j < cnt; ++j) ss += (int)line[j * C] * k[j];
    tmp[e] = (uint8_t)clip8(ss >> 22);
  }
  __syncthreads();
  const int n2 = Ho * WoC;
  for (int e = threadIdx.x; e < n2; e += DF_T) {
    const int y = e / WoC, xc = e - y * WoC;
    const int y0 = vb[2 * y], cnt = vb[2 * y + 1];
    const uint8_t* col = tmp + (y0 - r0) * WoC + xc;
    const int* k = vk + (int64_t)y * vks;
    int ss = 1 << 21;
    for (int j = 0; j < cnt; ++j) ss += (int)col[j * WoC] * k[j];
    out[e] = (uint8_t)clip8(ss >> 22);
  }
}

static FuncAttrLatch g_resize_lds;

// The address of kFetchTable on the current device, for the kernels of image_feed.hip: they write the same 256 values and read
// them from this one table (a __constant__ of another translation unit is not visible to them without relocatable device code).
hipError_t fetch_table_device(const float** table) {
  void* p = nullptr;
  hipError_t e = hipGetSymbolAddress(&p, HIP_SYMBOL(kFetchTable));
  *table = reinterpret_cast<const FetchTable*>(p)->v;
  return e;
}

}  // namespace diagan

using namespace diagan;

DIAGAN_API int diagan_data_fetch_table(float* table_host) {
  DG_REQUIRE(table_host != nullptr, "diagan_data_fetch_table: null output");
  for (int i = 0; i < 256; ++i) table_host[i] = kFetchTableHost.v[i];
  return DIAGAN_OK;
}

DIAGAN_API int diagan_data_fetch(const void* src, int64_t N, int H, int W, int C, const int64_t* idx, int64_t lo, int B,
                                 float* dst, void* stream) {
  DG_REQUIRE(src != nullptr && dst != nullptr, "diagan_data_fetch: null pointer");
  DG_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && B >= 0, "diagan_data_fetch: bad shape N=%ld H=%d W=%d C=%d B=%d", (long)N, H, W, C, B);
  DG_REQUIRE((int64_t)H * W * C < (1LL << 31), "diagan_data_fetch: one image of %d x %d x %d exceeds 2^31 bytes", H, W, C);
  DG_REQUIRE(idx != nullptr || (lo >= 0 && lo + B <= N), "diagan_data_fetch: range [%ld, %ld) outside [0, %ld)", (long)lo,
             (long)(lo + B), (long)N);
  if (B == 0) return DIAGAN_OK;
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  const uint8_t* in = (const uint8_t*)src;
  const bool aligned = ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 15) == 0;      // 4-byte loads, 16-byte stores
  if (HW % 4 == 0 && (C == 1 || C == 3) && aligned) {
    const int blocks = (int)std::min<int64_t>(DF_MAX_BLOCKS, ((int64_t)B * (HW / 4) + DF_T - 1) / DF_T);
    if (C == 1)
      hipLaunchKernelGGL(data_fetch_quad_kernel<1>, dim3(blocks), dim3(DF_T), 0, s, in, idx, lo, B, HW, dst);
    else
      hipLaunchKernelGGL(data_fetch_quad_kernel<3>, dim3(blocks), dim3(DF_T), 0, s, in, idx, lo, B, HW, dst);
  } else {
    const int blocks = (int)std::min<int64_t>(DF_MAX_BLOCKS, ((int64_t)B * C * HW + DF_T - 1) / DF_T);
    hipLaunchKernelGGL(data_fetch_scalar_kernel, dim3(blocks), dim3(DF_T), 0, s, in, idx, lo, B, HW, C, dst);
  }
  return check_launch("diagan_data_fetch");
}

DIAGAN_API int diagan_data_resize_crop(const void* src, int n, int Hs, int Ws, int C, void* dst, int Ho, int Wo, const int* hb,
                                       const int* hk, int hks, const int* vb, const int* vk, int vks, int r0, int r1,
                                       void* stream) {
  DG_REQUIRE(src != nullptr && dst != nullptr && hb != nullptr && hk != nullptr && vb != nullptr && vk != nullptr,
             "diagan_data_resize_crop: null pointer");
  DG_REQUIRE(n >= 0 && Hs > 0 && Ws > 0 && C > 0 && Ho > 0 && Wo > 0 && hks > 0 && vks > 0,
             "diagan_data_resize_crop: bad shape n=%d %dx%dx%d -> %dx%d", n, Hs, Ws, C, Ho, Wo);
  DG_REQUIRE(0 <= r0 && r0 < r1 && r1 <= Hs, "diagan_data_resize_crop: source rows [%d, %d) outside [0, %d)", r0, r1, Hs);
  DG_REQUIRE((int64_t)Hs * Ws * C < (1LL << 31) && (int64_t)Ho * Wo * C < (1LL << 31), "diagan_data_resize_crop: image too large");
  const int64_t lds = (int64_t)(r1 - r0) * Wo * C;
  if (lds > 160 * 1024)
    return set_err(DIAGAN_EUNSUP, "diagan_data_resize_crop: %ld bytes of intermediate rows exceed the 160 KiB of LDS", (long)lds);
  if (n == 0) return DIAGAN_OK;
  DG_LDS(g_resize_lds, data_resize_crop_kernel, (size_t)lds);
  hipLaunchKernelGGL(data_resize_crop_kernel, dim3(n), dim3(DF_T), (size_t)lds, (hipStream_t)stream, (const uint8_t*)src, Hs, Ws, C,
                     (uint8_t*)dst, Ho, Wo, hb, hk, hks, vb, vk, vks, r0, r1);
  return check_launch("diagan_data_resize_crop");
}
