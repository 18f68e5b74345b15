/* libdiagan_hip.so -- LPIPS (the learned perceptual image patch similarity, VGG16 variant) for the perceptual path length
 * (DESIGN.md section 8n).
 *
 * The 13 VGG16 convolutions run on diagan_incep_conv (include/diagan_hip.h); this header adds what that network lacks: the
 * input preparation with the scaling layer and a crop window, the 2 x 2 max pool, the sum of a convolution's partial results
 * over blocks of input channels, and the distance head of one tap.
 *
 * Same conventions and the same prototype grammar as include/diagan_hip.h (this file is read by diagan/_native/lpips_abi.py the
 * way that one is read by diagan/_native): plain C types, device pointers owned by the caller, 0 or a negative DIAGAN_E* code with
 * the text in diagan_last_error(), launch on `stream`, no synchronisation, no allocation.  Every output element is formed by one
 * thread or one workgroup in an order fixed by the image's shape alone (no atomics, nothing depends on B): reruns are
 * bit-identical and an image's value does not depend on the batch it is in.
 * Every name here starts with diagan_lpips_ and returns int, except the workspace query.
 */
#ifndef DIAGAN_LPIPS_H
#define DIAGAN_LPIPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* x fp32 [B][3][H][W] (or [B][H][W][3] with nhwc) -> y fp32 [B][h][w][4]: the window of h x w pixels whose first pixel is
 * (y0, x0) -- (0, 0, H, W) is the whole image -- through the scaling layer, y_c = (x_c - shift_c) / scale_c with
 * shift = (-.030, -.088, -.188) and scale = (.458, .448, .450) as fp32 constants, one fp32 subtraction and one fp32 division;
 * channel 3 = 0.  scale == 0 copies the window unscaled (LPIPS version '0.0').  0 <= y0, y0 + h <= H, 0 <= x0, x0 + w <= W. */
int diagan_lpips_prep(const float* x, int nhwc, int B, int H, int W, int y0, int x0, int h, int w, int scale, float* y,
                      void* stream);

/* 2 x 2 max pool with stride 2 over NHWC: x [B][H][W][C] -> y [B][H / 2][W / 2][C], the odd last row and column dropped
 * (nn.MaxPool2d(2, 2)).  C a multiple of 4, H, W >= 2, x and y 16-byte aligned.  PRECONDITION: no NaN in x. */
int diagan_lpips_pool2(const float* x, int B, int H, int W, int C, float* y, void* stream);

/* Blocked summation of a convolution over its input channels.  diagan_incep_conv adds its R S Ci products one after the other
 * into one fp32 accumulator; over 9 x 512 terms that rounding walk is three to four times the error of a sum taken in blocks, and
 * the perceptual path length measures feature DIFFERENCES of 1e-4.  So a VGG16 layer runs once per block of input channels, each
 * launch writing its partial result into its channel slice of parts [N][nparts][C] (no bias, no ReLU), and this launch forms
 *   y[n][c] = act((float)(bias[c] + parts[n][0][c] + ... + parts[n][nparts - 1][c])),
 * the sum in float64 in block order, rounded to fp32 once; act = ReLU when relu.  N pixels (B H W), C a multiple of 4; parts,
 * bias and y 16-byte aligned. */
int diagan_lpips_sum_parts(const float* parts, int64_t N, int C, int nparts, const float* bias, int relu, float* y, void* stream);

/* Bytes of workspace diagan_lpips_head needs (0 for a shape it refuses).  Host logic only. */
size_t diagan_lpips_head_ws_bytes(int B, int H, int W, int C);

/* The distance head of one tap, in one read of the two feature maps:
 *   d[b] = 1 / (H W) sum_p sum_c w[c] (f0[b][p][c] / (|f0[b][p]| + 1e-10) - f1[b][p][c] / (|f1[b][p]| + 1e-10))^2,
 * |.| the channel norm at pixel p; out[b] = d[b], or out[b] += d[b] when add.  out is FLOAT64 [B].
 * Image b of f0 starts at f0 + b * image_stride (elements), likewise f1: two tensors have image_stride = H W C; the pairs of an
 * interleaved [2B][H][W][C] batch are f0 = base, f1 = base + H W C, image_stride = 2 H W C.  image_stride >= H W C.
 * The features are fp32; everything after the load is float64: both sums of squares, the square root, the reciprocal of
 * (norm + 1e-10) -- one division per pixel and map; each element is then multiplied by it --, the difference, the weighted sum
 * and the sum over pixels.  The difference is taken element by element (the expanded form with the three dot products cancels
 * to nothing for near pairs and is not used); products and sums are rounded separately, so identical maps give exactly 0.
 * A pixel whose features are all zero contributes 0.
 * A lane group owns a pixel (16-byte loads, shuffles across the group); a workgroup sums a fixed run of pixels into ws, a second
 * launch sums an image's partials in index order.  C a multiple of 4, 4 <= C <= 1024; H, W >= 1; f0, f1, w 16-byte aligned and
 * image_stride a multiple of 4; ws 8-byte aligned with ws_bytes >= diagan_lpips_head_ws_bytes(B, H, W, C). */
int diagan_lpips_head(const float* f0, const float* f1, int64_t image_stride, int B, int H, int W, int C, const float* w,
                      double* out, int add, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
