// Stand-alone host check of csrc/gemm_x3_halo.h, the LDS layout of the resident-image form of the split-operand lone-tile GEMM
// (csrc/conv_gemm_x3.hip).  No GPU, no HIP: build with the host compiler and run, e.g.
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I self-diagnosing-gan_amd/csrc \
//         tools/host/gemm_x3_halo_check.cpp -o /tmp/gemm_x3_halo_check && /tmp/gemm_x3_halo_check
// (tests/test_gemm_x3_halo_host.py does exactly that).  It replays the kernel's staging and its fragment reads on a host array of the
// LDS image's size, so an index outside the image is an out-of-bounds access for the sanitizer as well as a failed check here.
#include "gemm_x3_halo.h"

#include <cstdio>
#include <set>
#include <vector>

using namespace diagan;

static int fails = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++fails <= 20) { std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                     \
  } while (0)

// lane groups one ds_read_b128 is served in (a 32-lane half; the other half reads another plane in groups of its own)
static const int kGroups[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                   {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};

static void check_ci(int Ci, int dr, int off) {
  const int hpix = gxr_pix_pitch(Ci), hrow = gxr_row_pitch(Ci), plane = gxr_plane(Ci);
  CHECK(hrow >= GXR_HALO * hpix, "Ci %d: rows overlap", Ci);
  CHECK((hpix * 2) % 16 == 0 && (hrow * 2) % 16 == 0, "Ci %d: 16-byte alignment", Ci);
  CHECK(((hrow * 2 / 16) & 15) == 8, "Ci %d: row pitch %d slots", Ci, hrow * 2 / 16);
  // ---- staging, as the kernel does it: ring of zeros, interior = pixel id + 1 per channel chunk; the rest stays "dirty" ----
  std::vector<int> img(plane, -1);
  const int cq = Ci / 8;
  std::set<int> ring;
  for (int i = 0; i < GXR_BORDER * cq; ++i) {
    const int bp = i / cq, ch = i - bp * cq;
    int hy, hx;
    gxr_border_pixel(bp, hy, hx);
    CHECK(hy >= 0 && hy < GXR_HALO && hx >= 0 && hx < GXR_HALO && (hy == 0 || hy == GXR_HALO - 1 || hx == 0 || hx == GXR_HALO - 1),
          "ring pixel %d = (%d, %d)", bp, hy, hx);
    ring.insert(hy * GXR_HALO + hx);
    for (int e = 0; e < 8; ++e) img.at(hy * hrow + hx * hpix + ch * 8 + e) = 0;
  }
  CHECK((int)ring.size() == GXR_BORDER, "ring has %d pixels", (int)ring.size());
  for (int i = 0; i < 64 * cq; ++i) {
    const int pix = i / cq, ch = i - pix * cq;
    const int d = ((pix >> 3) + 1) * hrow + ((pix & 7) + 1) * hpix + ch * 8;
    CHECK(d == gxr_halo_off(pix, 0, 0, 1, -1, Ci) + hrow + hpix + ch * 8, "interior slot of pixel %d", pix);
    for (int e = 0; e < 8; ++e) {
      CHECK(img.at(d + e) == -1, "Ci %d: pixel %d chunk %d written twice", Ci, pix, ch);
      img.at(d + e) = 1 + pix;
    }
  }
  // ---- every tap's fragment reads: 64 pixels x 9 taps x every K-step's four 8-channel blocks ----
  for (int r = 0; r < 3; ++r)
    for (int s = 0; s < 3; ++s) {
      const int dy = off + r * dr, dx = off + s * dr;         // the gather formula of conv_common.h
      for (int pix = 0; pix < 64; ++pix) {
        const int hp = gxr_halo_pixel(pix, r, s, dr, off);
        CHECK(hp >= 0 && hp < GXR_HALO * GXR_HALO, "halo pixel %d of pixel %d tap (%d, %d)", hp, pix, r, s);
        const int iy = (pix >> 3) + dy, ix = (pix & 7) + dx;
        const bool inside = iy >= 0 && iy < GXR_HW && ix >= 0 && ix < GXR_HW;
        const int want = inside ? 1 + iy * GXR_HW + ix : 0;   // the image shifted by the tap, zero outside
        CHECK(inside ? hp == (iy + 1) * GXR_HALO + ix + 1 : ring.count(hp) == 1, "pixel %d tap (%d, %d) -> halo %d", pix, r, s, hp);
        // the kernel's address: the lane's offset for tap (0, 0) of a forward gather + the step's uniform offset
        const int lane_off = gxr_halo_off(pix, 0, 0, 1, -1, Ci);
        const int step_off = (1 + off + r * dr) * hrow + (1 + off + s * dr) * hpix;
        CHECK(lane_off + step_off == gxr_halo_off(pix, r, s, dr, off, Ci), "offset split of pixel %d", pix);
        for (int c = 0; c < Ci; c += 8)
          for (int e = 0; e < 8; ++e) {
            const int o = lane_off + step_off + c + e;
            CHECK(o >= 0 && o < plane && img.at(o) == want, "Ci %d pixel %d tap (%d, %d) channel %d reads %d, wants %d", Ci, pix, r, s,
                  c + e, (o >= 0 && o < plane) ? img[o] : -2, want);
          }
      }
      // ---- banks: each 16-lane group of a fragment read (rows wm * 32 + lane) on 16 different 16-byte slots of the 256-byte row ----
      for (int wm = 0; wm < 2; ++wm)
        for (int grp = 0; grp < 2; ++grp)
          for (int c = 0; c < Ci; c += 8) {
            std::set<int> slots;
            for (int l = 0; l < 16; ++l) slots.insert(((gxr_halo_off(wm * 32 + kGroups[grp][l], r, s, dr, off, Ci) + c) * 2 / 16) & 15);
            CHECK(slots.size() == 16, "Ci %d tap (%d, %d) wm %d group %d: %d slots", Ci, r, s, wm, grp, (int)slots.size());
          }
    }
}

int main() {
  int max_ci = 0;
  for (int Ci = 32; Ci <= 1024; Ci += 32) {
    const bool ok = gxr_shape_ok(4, 8, 8, Ci, 8, 8, 3, 3, 1, -1);
    CHECK(ok == (gxr_lds_bytes(Ci) <= GXR_LDS_MAX), "Ci %d: predicate against the LDS size", Ci);
    if (ok) {
      CHECK(max_ci == Ci - 32, "the accepted Ci are not one range");
      max_ci = Ci;
      check_ci(Ci, 1, -1);
      check_ci(Ci, -1, 1);
    }
  }
  CHECK(max_ci == 128, "largest Ci %d (128 must fit; its image takes %ld bytes)", max_ci, gxr_lds_bytes(128));
  CHECK(gxr_lds_bytes(128) == 149760, "LDS bytes at Ci = 128: %ld", gxr_lds_bytes(128));
  // geometries that keep the per-tap form
  CHECK(!gxr_shape_ok(3, 6, 10, 64, 6, 10, 3, 3, 1, -1), "6 x 10 map");
  CHECK(!gxr_shape_ok(2, 4, 4, 256, 4, 4, 3, 3, 1, -1), "4 x 4 map");
  CHECK(!gxr_shape_ok(2, 4, 16, 64, 4, 16, 3, 3, 1, -1), "4 x 16 map: 64 pixels, but not 8 x 8");
  CHECK(!gxr_shape_ok(2, 8, 8, 64, 8, 8, 1, 1, 1, 0), "1 x 1");
  CHECK(!gxr_shape_ok(2, 8, 8, 64, 8, 8, 3, 3, 1, 0), "pad 0");
  CHECK(!gxr_shape_ok(2, 8, 8, 64, 8, 8, 3, 3, -1, -1), "mixed signs");
  CHECK(!gxr_shape_ok(2, 8, 8, 48, 8, 8, 3, 3, 1, -1), "Ci not a multiple of 32");
  CHECK(!gxr_shape_ok(70000, 8, 8, 128, 8, 8, 3, 3, 1, -1), "byte offsets past 2^31");
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("gemm_x3_halo_check: OK (Ci up to %d)\n", max_ci);
  return 0;
}
