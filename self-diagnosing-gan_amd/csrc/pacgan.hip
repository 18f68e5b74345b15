// PacGAN packing: the discriminator of a packed pair sees p images at once, chunk j of the batch stacked
// on the channel axis behind chunk j - 1 (torch.cat(torch.split(x, B / p), dim=1) of the reference's MNIST_DCGAN_Discriminator).
// In this engine's layout -- fp32 NHWC, channel counts padded to a multiple of 4 -- that is
//   pac_pack_kernel     x [B][HW][Cp] or src [B][nc][HW]  ->  out [n][HW][Cq],  out[b][s][j nc + c] = x[j n + b][s][c]
//   pac_unpack_kernel   g [n][HW][Cq]                     ->  gx [B][HW][Cp],   gx[j n + b][s][c]  = g[b][s][j nc + c]
// with n = B / p, Cp = r4(nc), Cq = r4(nc p).  The lanes that carry no channel (nc p .. Cq - 1 of out, nc .. Cp - 1 of gx) are
// written as 0.0f: the first convolution's padded weight columns and the generator's tanh backward read them.
//
// Pure data movement: every value keeps its bits.  One thread forms one 16-byte group of the OUTPUT and stores it once; the four
// lanes of a group are looked up one by one, because a group of the packed tensor straddles source images (nc = 3, p = 2: lane 3
// of the first group is channel 0 of chunk 1).  Grid-stride, 64-bit element offsets.  Roofline: HBM; at the sizes of a training
// step (64 x 32 x 32 x 4 floats = 1 MiB) the launch itself is what it costs.
#include "common.h"
#include "diagan_lpips.h"

namespace diagan {

using pf4 = __attribute__((ext_vector_type(4))) float;

constexpr int PAC_T = 256;
static inline int pac_blocks(int64_t n) {
  int64_t b = (n + PAC_T - 1) / PAC_T;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));      // grid-stride beyond 8192 blocks
}

// NCHW: the source is [B][nc][HW] (channel stride HW); otherwise [B][HW][Cp] (channel stride 1)
template <bool NCHW>
__global__ __launch_bounds__(PAC_T) void pac_pack_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t ngroups,
                                                         int64_t n, int64_t HW, int nc, int Cp, int p, int Cq) {
  const int q4 = Cq >> 2, live = nc * p;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ngroups; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pix = i / q4;                 // b HW + s
    const int q = (int)(i - pix * q4);
    const int64_t b = pix / HW, s = pix - b * HW;
    pf4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int l = q * 4 + e;
      float t = 0.0f;
      if (l < live) {
        const int j = l / nc, c = l - j * nc;
        const int64_t img = (int64_t)j * n + b;
        t = NCHW ? x[(img * nc + c) * HW + s] : x[(img * HW + s) * Cp + c];
      }
      v[e] = t;
    }
    reinterpret_cast<pf4*>(out)[i] = v;
  }
}

__global__ __launch_bounds__(PAC_T) void pac_unpack_kernel(const float* __restrict__ g, float* __restrict__ gx, int64_t ngroups,
                                                           int64_t n, int64_t HW, int nc, int Cp, int Cq) {
  const int p4 = Cp >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ngroups; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pix = i / p4;                 // (j n + b) HW + s
    const int q = (int)(i - pix * p4);
    const int64_t img = pix / HW, s = pix - img * HW;
    const int64_t j = img / n, b = img - j * n;
    const float* row = g + (b * HW + s) * Cq + j * nc;
    pf4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = q * 4 + e;
      v[e] = c < nc ? row[c] : 0.0f;
    }
    reinterpret_cast<pf4*>(gx)[i] = v;
  }
}

// the checks the three entry points share; 0 or the negative code with the text set
static int pac_check(const char* who, const void* a, const void* b, int B, int H, int W, int nc, int Cp, int p, int Cq) {
  DG_REQUIRE(a != nullptr && b != nullptr, "%s: null pointer", who);
  DG_REQUIRE(B >= 1 && H >= 1 && W >= 1 && nc >= 1, "%s: bad shape B=%d H=%d W=%d nc=%d", who, B, H, W, nc);
  DG_REQUIRE(p >= 1, "%s: num_pack p=%d must be at least 1", who, p);
  DG_REQUIRE(B % p == 0, "%s: batch B=%d is not a multiple of num_pack p=%d", who, B, p);
  DG_REQUIRE(Cp == ((nc + 3) & ~3), "%s: Cp=%d is not nc=%d rounded up to a multiple of 4", who, Cp, nc);
  DG_REQUIRE((int64_t)nc * p <= Cq, "%s: Cq=%d is smaller than nc * p = %d * %d", who, Cq, nc, p);
  DG_REQUIRE((Cq & 3) == 0, "%s: Cq=%d is not a multiple of 4", who, Cq);
  return DIAGAN_OK;
}

}  // namespace diagan

using namespace diagan;

DIAGAN_API int diagan_pac_pack(const float* x, int B, int H, int W, int nc, int Cp, int p, int Cq, float* out, void* stream) {
  if (int rc = pac_check("diagan_pac_pack", x, out, B, H, W, nc, Cp, p, Cq)) return rc;
  DG_REQUIRE(((uintptr_t)out & 15) == 0, "diagan_pac_pack: out must be 16-byte aligned");
  const int64_t n = B / p, HW = (int64_t)H * W, ngroups = n * HW * (Cq / 4);
  hipLaunchKernelGGL(pac_pack_kernel<false>, dim3(pac_blocks(ngroups)), dim3(PAC_T), 0, (hipStream_t)stream, x, out, ngroups, n, HW,
                     nc, Cp, p, Cq);
  return check_launch("diagan_pac_pack");
}

DIAGAN_API int diagan_pac_pack_nchw(const float* src, int B, int nc, int H, int W, int p, int Cq, float* out, void* stream) {
  if (int rc = pac_check("diagan_pac_pack_nchw", src, out, B, H, W, nc, (nc + 3) & ~3, p, Cq)) return rc;
  DG_REQUIRE(((uintptr_t)out & 15) == 0, "diagan_pac_pack_nchw: out must be 16-byte aligned");
  const int64_t n = B / p, HW = (int64_t)H * W, ngroups = n * HW * (Cq / 4);
  hipLaunchKernelGGL(pac_pack_kernel<true>, dim3(pac_blocks(ngroups)), dim3(PAC_T), 0, (hipStream_t)stream, src, out, ngroups, n, HW,
                     nc, 0, p, Cq);
  return check_launch("diagan_pac_pack_nchw");
}

DIAGAN_API int diagan_pac_unpack(const float* g, int B, int H, int W, int nc, int Cp, int p, int Cq, float* gx, void* stream) {
  if (int rc = pac_check("diagan_pac_unpack", g, gx, B, H, W, nc, Cp, p, Cq)) return rc;
  DG_REQUIRE(((uintptr_t)gx & 15) == 0, "diagan_pac_unpack: gx must be 16-byte aligned");
  const int64_t n = B / p, HW = (int64_t)H * W, ngroups = (int64_t)B * HW * (Cp / 4);
  hipLaunchKernelGGL(pac_unpack_kernel, dim3(pac_blocks(ngroups)), dim3(PAC_T), 0, (hipStream_t)stream, g, gx, ngroups, n, HW, nc,
                     Cp, Cq);
  return check_launch("diagan_pac_unpack");
}
