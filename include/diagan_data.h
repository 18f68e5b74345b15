/* libdiagan_hip.so -- second header of the C ABI: the device-resident dataset feed.
 *
 * The reference reads its datasets through torchvision: PIL transforms per item in loader workers, collate, pinned host-to-device
 * copy (diagan-pkg/diagan/datasets/predefined.py:30-36, transform.py).  Here a dataset is transformed once to uint8 NHWC at the
 * training size, kept in HBM, and turned into batches by one launch.
 *
 * Same conventions and the same prototype grammar as include/diagan_hip.h (this file is read by diagan/_native/data_abi.py the way
 * that one is read by diagan/_native): plain C types, device pointers owned by the caller unless a parameter says "host", 0 or a
 * negative DIAGAN_E* code with the text in diagan_last_error(), launch on `stream`, no synchronisation, no allocation.
 * Every name here starts with diagan_data_ and returns int.
 */
#ifndef DIAGAN_DATA_H
#define DIAGAN_DATA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ToTensor + Normalize(0.5, 0.5) of a batch (transform.py:9-10 and its three siblings) fused with the gather:
 *   dst[b][c][y][x] = (src[row_b][y][x][c] / 255 - 0.5) / 0.5,   row_b = idx ? idx[b] : lo + b
 * src uint8 [N,H,W,C]; idx int64 [B] (any order, repeats allowed) or NULL; dst fp32 [B,C,H,W].  Each value carries the bits of the
 * torch CPU sequence t.to(float32).div(255).sub(0.5).div(0.5).  Any H, W, C; planes of H*W % 4 == 0 with C of 1 or 3 take the
 * 16-byte-store kernel.  PRECONDITION: 0 <= idx[b] < N (the range form is checked here). */
int diagan_data_fetch(const void* src, int64_t N, int H, int W, int C, const int64_t* idx, int64_t lo, int B, float* dst,
                      void* stream);

/* The 256 values diagan_data_fetch can write, table_host[v] for byte v, copied to HOST memory (no device call). */
int diagan_data_fetch_table(float* table_host);

/* Resize(s) + CenterCrop(s) of the same transforms on uint8 images, bit-identical to PIL's Image.resize(..., BILINEAR) followed by
 * the crop: a horizontal pass, a rounded uint8 intermediate, a vertical pass, each clip8((2^21 + sum pix * k) >> 22).
 * src [n,Hs,Ws,C], dst [n,Ho,Wo,C] (the cropped size).  Tables for the KEPT output columns (hb, hk) and rows (vb, vk), int32:
 * bounds [out][2] = (first source index, number of taps), coefficients [out][ks]; a pass that PIL skips (size unchanged) is the
 * table with one tap of 2^22.  [r0, r1): the source rows the kept output rows read; (r1 - r0)*Wo*C bytes of LDS, at most 160 KiB.
 * PRECONDITION: every (first, taps) lies inside the source (columns in [0, Ws), rows in [r0, r1)) and taps <= ks. */
int diagan_data_resize_crop(const void* src, int n, int Hs, int Ws, int C, void* dst, int Ho, int Wo, const int* hb, const int* hk,
                            int hks, const int* vb, const int* vk, int vks, int r0, int r1, void* stream);

#ifdef __cplusplus
}
#endif
#endif
