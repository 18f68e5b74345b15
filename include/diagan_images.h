/* libdiagan_hip.so -- the image feed of the StyleGAN2 trainers.
 *
 * The reference packs an image folder into an lmdb of Lanczos-resized JPEGs (stylegan2/prepare_data.py), reads it item by item
 * (stylegan2/dataset.py) and flips, converts and normalises each item on the host (train_ffhq.py:588-600).  Here the packed set is
 * uint8 NHWC in HBM (section 8j), the flip moves into the fetch, and the ingest resize works band by band so that a source of any
 * height fits the LDS.
 *
 * Same conventions and the same prototype grammar as include/diagan_hip.h (this file is read by diagan/_native/img_abi.py the way
 * that one is read by diagan/_native): plain C types, device pointers owned by the caller unless a parameter says "host", 0 or a
 * negative DIAGAN_E* code with the text in diagan_last_error(), launch on `stream`, no allocation on the device.
 * Every name here starts with diagan_img_ and returns int.
 */
#ifndef DIAGAN_IMAGES_H
#define DIAGAN_IMAGES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* RandomHorizontalFlip + ToTensor + Normalize(0.5, 0.5) of a batch (train_ffhq.py:588-594) fused with the gather:
 *   dst[b][c][y][x] = T[src[row_b][y][flip[b] ? W-1-x : x][c]],   row_b = idx ? idx[b] : lo + b
 * T is the 256-entry table of diagan_data_fetch (diagan_data_fetch_table returns it): the same device table, not a copy.
 * src uint8 [N,H,W,C]; idx int64 [B] (any order, repeats allowed) or NULL; flip uint8 [B] (non-zero: mirror the item) or NULL for
 * "no flip", which writes the bytes diagan_data_fetch writes; dst fp32 [B,C,H,W].  Any H, W, C; planes of H*W % 4 == 0 with C of
 * 1 or 3 take the 16-byte-store kernel.  No synchronisation.  PRECONDITION: 0 <= idx[b] < N (the range form is checked here). */
int diagan_img_fetch_flip(const void* src, int64_t N, int H, int W, int C, const int64_t* idx, int64_t lo, const void* flip, int B,
                          float* dst, void* stream);

/* diagan_data_resize_crop for sources of any height: the same two passes -- horizontal first, a rounded uint8 intermediate, then
 * vertical, each clip8((2^21 + sum pix * k) >> 22) -- and the same tables (int32 bounds [out][2] = (first source index, taps),
 * coefficients [out][ks] scaled by 2^22, for the KEPT output columns and rows), one workgroup per (image, band of band_rows
 * output rows).  A workgroup keeps in LDS the horizontal pass of only the source rows its band reads, [min first, max first+taps)
 * over the band's rows of vb: 16 + rows*Wo*C bytes.  A band that needs more than 160 KiB returns DIAGAN_EUNSUP with the byte
 * count and nothing is launched.  Ho % band_rows != 0 is legal (the last band is short).  src [n,Hs,Ws,C], dst [n,Ho,Wo,C].
 * Coefficients may be negative (Lanczos lobes); sums are int32, see the bound below.
 * This entry point, alone in the library, reads a device table back: vb (8*Ho bytes) is copied to the host on `stream` and the
 * stream is awaited, to size the LDS and to check every vertical (first, taps) against [0, Hs) and vks before the launch.  It is
 * ingest, not the training loop.
 * PRECONDITION: every horizontal (first, taps) lies inside [0, Ws) with taps <= hks; in every row of hk and vk the positive
 * coefficients sum to at most 2^23 (then |2^21 + sum pix * k| <= 2^21 + 255 * 2^23 < 2^31; tables normalised to 2^22 with
 * negative lobes below 2^22 in total satisfy it). */
int diagan_img_resize_crop_banded(const void* src, int n, int Hs, int Ws, int C, void* dst, int Ho, int Wo, const int* hb,
                                  const int* hk, int hks, const int* vb, const int* vk, int vks, int band_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif
