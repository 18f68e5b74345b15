// LDS layout of the resident-image form of the split-operand lone-tile GEMM (conv_gemm_x3.hip: conv_gemm_x3_kernel_resident).
// Plain integer arithmetic, shared by the kernel, its host-side predicate and the stand-alone check tools/host/gemm_x3_halo_check.cpp
// (no HIP type in here: that program is built by the host compiler alone).
//
// A tile of the launches this form takes is ONE 8 x 8 image.  It sits in LDS once, as three bf16 piece planes of a 10 x 10 halo image
// (a ring of zero pixels = the padding of the 3 x 3 gather), and the A-fragment of tap (r, s) is the same 64 pixels read one halo
// row / column further on.
#pragma once

#if defined(__HIPCC__)
#define GXR_HD __host__ __device__ inline
#else
#define GXR_HD inline
#endif

namespace diagan {

constexpr int GXR_HW = 8;                          // the image: 8 x 8 pixels, the 64 rows of a tile
constexpr int GXR_HALO = GXR_HW + 2;               // ... with its ring of zeros
constexpr int GXR_BORDER = 4 * GXR_HW + 4;         // pixels of the ring (36)
constexpr int GXR_WSTAGE = 3 * 64 * 40;            // one weight stage: three piece planes [64 rows][40 bf16] (conv_gemm_x3.hip: GX_PLANE)
constexpr int GXR_LDS_MAX = 160 * 1024;            // dynamic LDS a workgroup can have

// Pitches in bf16 elements.  A fragment read is one ds_read_b128 per lane: lane fi of a 32-lane half reads 16 bytes of halo pixel
// (y0 + fi / 8, x0 + fi % 8); the hardware serves the half as two groups of 16 lanes, {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31},
// and a group is conflict-free when its 16 addresses fall on the 16 different 16-byte slots of the 256-byte bank row.
//   pixel pitch = Ci / 8 + 1 slots = P, with P = 1 (mod 4) because Ci is a multiple of 32: four neighbouring pixels of a row take
//     the slot set A = {0, P, 2P, 3P}, one slot of each residue mod 4, and the next four take A + 4P = A + 4 (mod 16);
//   row pitch = 8 (mod 16) slots: the first group reads columns 0-3 of image row 0, 4-7 of rows 1 and 2, 0-3 of row 3, i.e. the slots
//     A, A + 4 + 8, A + 4 + 16, A + 24 = A, A + 12, A + 4, A + 8 -- all 16; the second group the complement, A + 4, A + 8, A, A + 12.
//   (10 pixels of pitch P alone give a row pitch of 10 P = 10 (mod 16) at Ci = 128: the two middle rows of a group would meet the
//    outer ones on two slots each.)  The tap's (r, s) and the 8-channel block move every lane by the same amount.
GXR_HD int gxr_pix_pitch(int Ci) { return Ci + 8; }
GXR_HD int gxr_row_pitch(int Ci) {
  const int slots = GXR_HALO * (Ci / 8 + 1);
  return (slots + ((8 - slots) & 15)) * 8;
}
GXR_HD int gxr_plane(int Ci) { return GXR_HALO * gxr_row_pitch(Ci); }
// the whole workgroup: 2 K-groups x 2 weight stages, then the three halo planes (bytes).  Ci = 128: 61 440 + 88 320 = 149 760
GXR_HD long gxr_lds_bytes(int Ci) { return (4L * GXR_WSTAGE + 3L * gxr_plane(Ci)) * 2; }

// halo pixel (its index in the 10 x 10 image) that row `pix` of the tile gathers for tap (r, s) of the gather formula of conv_common.h,
// iy = oy + off + r * dr: forward (dr, off) = (1, -1), data gradient (-1, 1)
GXR_HD int gxr_halo_pixel(int pix, int r, int s, int dr, int off) {
  return ((pix >> 3) + 1 + off + r * dr) * GXR_HALO + (pix & 7) + 1 + off + s * dr;
}
// the same as an element offset into a piece plane
GXR_HD int gxr_halo_off(int pix, int r, int s, int dr, int off, int Ci) {
  return ((pix >> 3) + 1 + off + r * dr) * gxr_row_pitch(Ci) + ((pix & 7) + 1 + off + s * dr) * gxr_pix_pitch(Ci);
}
// the i-th pixel of the ring, as (row, column) of the halo image: top row, bottom row, left column, right column
GXR_HD void gxr_border_pixel(int i, int& hy, int& hx) {
  if (i < GXR_HALO) { hy = 0; hx = i; }
  else if (i < 2 * GXR_HALO) { hy = GXR_HALO - 1; hx = i - GXR_HALO; }
  else if (i < 2 * GXR_HALO + GXR_HW) { hy = i - 2 * GXR_HALO + 1; hx = 0; }
  else { hy = i - 2 * GXR_HALO - GXR_HW + 1; hx = GXR_HALO - 1; }
}

// geometry of the resident form, beyond what gemm_x3_geom_ok asks: the 3 x 3 / pad 1 same-size gather (forward or data gradient) on
// 8 x 8 maps, the layout above inside the LDS (Ci <= 128), and byte offsets into the gathered tensor that fit the buffer descriptor
GXR_HD bool gxr_shape_ok(int B, int Hi, int Wi, int Ci, int Ho, int Wo, int R, int S, int dr, int off) {
  return R == 3 && S == 3 && ((dr == 1 && off == -1) || (dr == -1 && off == 1)) && Hi == GXR_HW && Wi == GXR_HW && Ho == GXR_HW &&
         Wo == GXR_HW && Ci > 0 && (Ci & 31) == 0 && gxr_lds_bytes(Ci) <= GXR_LDS_MAX && (long)B * 64 * Ci * 4 < (1L << 31);
}

}  // namespace diagan
