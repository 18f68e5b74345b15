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
 * Every name of this part starts with diagan_lpips_ and returns int, except the workspace query.  The head of the attribute
 * classifier, which runs on the same VGG16 feature extractor, follows (diagan_attr_*), and at the end of the file the PacGAN
 * packing of the MNIST-DCGAN discriminator (diagan_pac_*), which shares nothing with VGG16 but this binding table, and the head
 * of the SimpleConvNet group classifier (diagan_cls_*), which shares the loss with the attribute classifier.
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

/* ---- the head of the CelebA attribute classifier, a VGG16 with a two-class last layer ------------------
 *
 * The classifier's 13 convolutions run on diagan_incep_conv and its five max pools on diagan_lpips_pool2 above; the entry points
 * below add what its head needs: AdaptiveAvgPool2d((7, 7)) with the flatten, a dense layer wider than one output with its data
 * gradient and a weight gradient that carries the SGD step, the softmax cross-entropy and the count of the rows that show the
 * attribute.  They are declared in this header because it is the one diagan/_native/lpips_abi.py binds: the VGG16 family shares
 * one table.  Same conventions as above.  All tensors are fp32, row-major and contiguous unless stated.  No atomics: every
 * output element is formed by one thread or one workgroup in an order fixed by the shapes alone, so reruns are bit-identical; in
 * the forward pass a row's values do not depend on the other rows of the batch.  Every name starts with diagan_attr_ and returns int.
 *
 * A dense layer here is  Y[M][N] = act(X[M][K] W[N][K]^T + b[N]) * keep,  act = ReLU or nothing, keep = mask * drop_scale with
 * the 0 / 1 mask as bernoulli_ wrote it and drop_scale = 1 / (1 - p) (the convention of diagan_act_fwd), or 1 without a mask.
 * The gradient with respect to the pre-activation is  dZ = dY * [Y > 0] * keep  ([Y > 0] only for a ReLU layer, where the caller
 * passes Y; keep only where the caller passes the mask); the data gradient and the weight gradient form dZ while they load dY.
 */

/* nn.AdaptiveAvgPool2d((7, 7)) and the flatten, from NHWC: x [B][H][W][C] -> y [B][C 49] with y[b][c 49 + i 7 + j] the mean of
 * rows floor(i H / 7) .. ceil((i + 1) H / 7) - 1 and the same columns in j and W: torchvision's order.  The sum runs row by row
 * in fp32 and is divided by the bin's size once.  H, W in [1, 2^20]. */
int diagan_attr_pool_flatten(const float* x, int B, int H, int W, int C, float* y, void* stream);

/* The dense layer of the comment above.  bias may be NULL (none); relu != 0 applies ReLU; mask NULL means keep = 1.
 * N <= 4 takes a path of its own (a wave per row, N dot products); wider layers run on v_mfma_f32_16x16x4_f32 with exact fp32
 * products: a workgroup owns 16 columns and every row (128 rows per grid row for M > 128), its eight waves split K and add their
 * parts in wave order, so W is read from memory once.  K, N, M >= 1; 16-byte loads when K is a multiple of 4 and x and w are
 * 16-byte aligned, scalar loads otherwise. */
int diagan_attr_dense_fwd(const float* x, const float* w, const float* bias, int M, int K, int N, int relu, const float* mask,
                          float drop_scale, float* y, void* stream);

/* dX[M][K] = dZ[M][N] W[N][K],  dZ from dy [M][N] as above: y (the layer's output, NULL for a layer without ReLU), mask (NULL
 * for none) and drop_scale.  A workgroup owns 32 columns of K and every row; its four waves split N. */
int diagan_attr_dense_dgrad(const float* dy, const float* y, const float* mask, float drop_scale, const float* w, int M, int K,
                            int N, float* dx, void* stream);

/* The weight gradient and the optimiser step in one launch, M <= 128:
 *   g[n][k] = sum_m dZ[m][n] x[m][k],   buf_w = momentum buf_w + g,   w -= lr buf_w,
 * and the same for the bias with g[n] = sum_m dZ[m][n] (bias, buf_b NULL: a layer without bias).  With zero-initialised buffers
 * this is torch.optim.SGD(lr, momentum) with dampening 0, no Nesterov step and no weight decay.  The sum over the batch runs
 * in row order inside one wave; the gradient never reaches memory.  w is updated in place: launch it after the layer's data
 * gradient has read w.
 * g_w != NULL (with g_b, or g_b NULL to skip the bias) writes g there instead and leaves w, bias and the buffers alone: for tests. */
int diagan_attr_dense_wgrad_sgd(const float* dy, const float* y, const float* mask, float drop_scale, const float* x, int M, int K,
                                int N, float lr, float momentum, float* w, float* bias, float* buf_w, float* buf_b, float* g_w,
                                float* g_b, void* stream);

/* Softmax cross-entropy with mean reduction: logits [M][N], 1 <= N <= 64, targets int64 [M] in [0, N).
 *   dlogit[m][n] = (softmax(logits[m])[n] - [n == target[m]]) / M                       (fp32, computed in float64)
 *   loss_acc[0]    += 1 / M sum_m (log sum_n exp(z[m][n] - max_n z[m]) - (z[m][t] - max_n z[m]))      (float64 from the load on)
 *   correct_acc[0] += the number of rows whose FIRST maximum is at the target (torch.max(output, 1))
 * One workgroup; the accumulators are read and written by one thread, so successive launches on a stream add up. */
int diagan_attr_ce(const float* logits, const int64_t* target, int M, int N, float* dlogit, double* loss_acc,
                   int64_t* correct_acc, void* stream);

/* counter[0] += the number of rows of logits [M][N] whose first maximum is not at column 0 (a tie with column 0 counts as
 * class 0).  1 <= N <= 64.  One workgroup, as diagan_attr_ce. */
int diagan_attr_count(const float* logits, int M, int N, int64_t* counter, void* stream);

/* ---- PacGAN packing of the MNIST-DCGAN discriminator ----------------------------------------------------
 *
 * A discriminator built with num_pack = p judges p images at once: the batch of B images is cut into p chunks of n = B / p and
 * chunk j is stacked on the channel axis behind chunk j - 1 (torch.cat(torch.split(x, n), dim=1) in NCHW).  The three entry
 * points below are that rearrangement and its adjoint in this engine's layout, fp32 NHWC with padded channel counts:
 * Cp = nc rounded up to a multiple of 4 for the images, Cq a multiple of 4 and >= nc p (the first convolution's padded input
 * width) for the packed tensor.  They are declared in this header because the library's exports are the union of the headers
 * and diagan/_native/lpips_abi.py is the table that takes additions; nothing here touches VGG16.  Same conventions as above.
 * Pure data movement: every output value carries the bits of its source; one thread stores one 16-byte group of the output.
 * Refused before any launch: a null pointer, p < 1, B not a multiple of p, Cp != r4(nc), Cq < nc p or not a multiple of 4, an
 * output that is not 16-byte aligned.  Every name starts with diagan_pac_ and returns int.
 */

/* x [B][H][W][Cp] -> out [B / p][H][W][Cq]:  out[b][y][x][j nc + c] = x[j (B / p) + b][y][x][c]  for j < p, c < nc; the lanes
 * nc p .. Cq - 1 are written as 0.0f (the first convolution multiplies them by its padded weight columns). */
int diagan_pac_pack(const float* x, int B, int H, int W, int nc, int Cp, int p, int Cq, float* out, void* stream);

/* The same from src [B][nc][H][W] (NCHW, unpadded): diagan_nchw_to_nhwc and diagan_pac_pack in one launch, for the real batch. */
int diagan_pac_pack_nchw(const float* src, int B, int nc, int H, int W, int p, int Cq, float* out, void* stream);

/* The adjoint: g [B / p][H][W][Cq] -> gx [B][H][W][Cp],  gx[j (B / p) + b][y][x][c] = g[b][y][x][j nc + c]  for c < nc; the lanes
 * nc .. Cp - 1 are written as 0.0f (gx is the gradient of the generator's images: its tanh backward reads every lane). */
int diagan_pac_unpack(const float* g, int B, int H, int W, int nc, int Cp, int p, int Cq, float* gx, void* stream);

/* ---- the head of the SimpleConvNet group classifier -----------------------------------------------------
 *
 * The classifier's four 7 x 7 convolutions, their BatchNorm and the loss run on entry points that exist (diagan_conv_gemm,
 * diagan_bn_*, diagan_conv_wgrad, diagan_attr_ce); the three below add the end of the network: the last BatchNorm + ReLU, the
 * global mean, Linear(C, N) and F.normalize in one read of the last convolution's output, the adjoint of the mean and the linear
 * layer, and the histogram of the predicted labels.  Conventions of the diagan_attr_* section: fp32, row-major, contiguous, no
 * atomics, no allocation; every output element is formed in an order fixed by the shapes alone, and in the forward pass a row's
 * values do not depend on the other rows of the batch.  Every name starts with diagan_cls_ and returns int.
 */

/* x [B][HW][C], the last convolution's raw output; scale, shift [C] the BatchNorm of it as an affine map; w [N][C], bias [N].
 *   pooled[b][c] = (1 / HW) sum_p max(scale[c] x[b][p][c] + shift[c], 0)        (one fma per term; fp32 sums)
 *   logits[b][n] = sum_c pooled[b][c] w[n][c] + bias[n]                         (fp32)
 *   feat[b][c]   = pooled[b][c] / max(|pooled[b]|_2, 1e-12)                      (F.normalize(dim=1))
 * The norm is computed in FLOAT64: the squares, their sum and the square root; the division is a float64 division rounded to fp32
 * once.  An all-zero pooled row gives feat = 0.
 * A workgroup per image: 256 / (C / 4) rows of lanes each walk a fixed stride of the pixels with 16-byte loads, and the rows'
 * sums are added in row order.  C a multiple of 4, 4 <= C <= 1024; 1 <= N <= 64; HW >= 1; x, scale, shift 16-byte aligned.
 * logits may be NULL (then w and bias are not read), feat may be NULL; pooled is always written. */
int diagan_cls_head_fwd(const float* x, const float* scale, const float* shift, const float* w, const float* bias, int B, int HW,
                        int C, int N, float* pooled, float* logits, float* feat, void* stream);

/* The adjoint, from dlogit [B][N]:
 *   g[b][p][c] = (1 / HW) sum_n dlogit[b][n] w[n][c]   for every p, the sum with n ascending; the same bits at every p
 *   gw[n][c]   = sum_b dlogit[b][n] pooled[b][c],   gb[n] = sum_b dlogit[b][n],   b ascending
 * g is the gradient with respect to the ReLU's OUTPUT: the ReLU gate and the BatchNorm backward are diagan_bn_bwd(relu = 1) on g
 * and the saved x.  g may be NULL (weights only; then w is not read); gw and gb may each be NULL (then pooled is not read
 * without gw).  gw and gb are overwritten, not accumulated.  Same shape limits; B <= 65535; g 16-byte aligned. */
int diagan_cls_head_bwd(const float* dlogit, const float* w, const float* pooled, int B, int HW, int C, int N, float* g, float* gw,
                        float* gb, void* stream);

/* counts[n] += the number of rows of logits [M][N] whose FIRST maximum is at column n (torch.max(dim=1)'s rule, as diagan_attr_ce
 * states it: only a greater value replaces the maximum).  counts int64 [N], 8-byte aligned; 1 <= N <= 64.  One workgroup; lane n
 * alone reads and writes counts[n], so successive launches on a stream add up. */
int diagan_cls_histogram(const float* logits, int M, int N, int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
