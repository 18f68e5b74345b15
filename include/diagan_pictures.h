/* libdiagan_hip.so -- the pictures: a batch of images tiled into one uint8 grid on the device.
 *
 * The reference writes every picture through torchvision 0.8.2 (the version of its environment.yml): make_grid tiles the batch,
 * save_image converts the grid to bytes and PIL encodes them.  Here the batch is in HBM already, and one launch normalises,
 * clamps, tiles, pads, quantises and turns NCHW into HWC, so that only the finished bytes cross to the host.
 *
 * CONTRACT: the bytes are those torchvision 0.8.2 produces when it runs on torch CPU fp32:
 *   norm_ip(img, lo, hi):  img.clamp_(min=lo, max=hi); img.add_(-lo).div_(hi - lo + 1e-5)
 *                          the divisor is formed in double, rounded to fp32 once, and applied as ONE correctly rounded fp32
 *                          division (not a multiplication by a reciprocal; later torchvisions divide by max(hi - lo, 1e-5),
 *                          which is not this contract);
 *   save_image:            grid.mul(255).add_(0.5).clamp_(0, 255) truncated to uint8, mul and add rounded separately (the
 *                          object file is built with -ffp-contract=off).
 * A CUDA run of the reference multiplies by a reciprocal in div_ and may differ by one in rare bytes; that cannot be pinned and is
 * out of scope.
 *
 * Same conventions and the same prototype grammar as include/diagan_hip.h (this file is read by diagan/_native/pic_abi.py the way
 * that one is read by diagan/_native): plain C types, device pointers owned by the caller unless a parameter says "host", 0 or a
 * negative DIAGAN_E* code with the text in diagan_last_error(), launch on `stream`, no synchronisation, no allocation.
 * Every name here starts with diagan_pic_ and returns int, except the workspace query.
 */
#ifndef DIAGAN_PICTURES_H
#define DIAGAN_PICTURES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* normalisation of diagan_pic_grid */
#define DIAGAN_PIC_NORM_NONE 0   /* the values as they are */
#define DIAGAN_PIC_NORM_RANGE 1  /* norm_ip with the host range (lo, hi) */
#define DIAGAN_PIC_NORM_DATA 2   /* norm_ip with the two device floats diagan_pic_minmax left */
/* byte conversion of diagan_pic_grid */
#define DIAGAN_PIC_BYTES_SAVE_IMAGE 0  /* trunc(clamp(v * 255 + 0.5, 0, 255)) */
#define DIAGAN_PIC_BYTES_TO_NUMPY 1    /* trunc(clip((v + 1) / 2, 0, 1) * 255): the reference's to_numpy_image, utils/plot.py:10-15 */

/* Bytes of workspace diagan_pic_minmax needs for n elements (0 for n < 1).  Host logic only. */
size_t diagan_pic_minmax_ws(int64_t n);

/* lohi[0] = min x, lohi[1] = max x over the fp32 array x of n >= 1 elements: two launches (partial extremes per workgroup into ws,
 * then one workgroup combines them), no atomics, so the result does not depend on the launch geometry.  ws_bytes >=
 * diagan_pic_minmax_ws(n), 4-byte aligned.  PRECONDITION: every element is finite. */
int diagan_pic_minmax(const float* x, int64_t n, float* lohi, void* ws, int64_t ws_bytes, void* stream);

/* The ONLY definition of the grid's size (make_grid's): xmaps = min(nrow, B), ymaps = ceil(B / xmaps),
 * hw_host[0] = Hg = ymaps * (H + padding) + padding, hw_host[1] = Wg = xmaps * (W + padding) + padding; B == 1 gives (H, W):
 * a single image comes back unpadded.  hw_host: two host ints.  Host logic only. */
int diagan_pic_grid_shape(int B, int H, int W, int nrow, int padding, int* hw_host);

/* x fp32 [B,C,H,W] -> out uint8 [Hg,Wg,3] of diagan_pic_grid_shape, in one launch.  C is 1 (the plane goes to all three channels)
 * or 3; any H, W >= 1, nrow >= 1, padding >= 0.  Image k sits at row k / xmaps, column k % xmaps; every other pixel, the cells of
 * an incomplete last row included, is pad_value, which goes through the byte conversion but not through the normalisation.
 *   norm    DIAGAN_PIC_NORM_*: NONE; RANGE uses the host doubles lo, hi; DATA reads lohi (device, two floats) inside the kernel,
 *           so nothing crosses to the host between diagan_pic_minmax and this launch.  lo, hi are ignored unless RANGE; lohi is
 *           ignored (may be NULL) unless DATA.
 *   passes  1, or 2: make_grid(normalize=True) followed by save_image(grid, normalize=True), as the reference's panels do
 *           (utils/plot.py:74-82).  The second norm_ip runs over the grid with lo2 = 0 and hi2 = the first pass's image of the
 *           maximum, computed from the same two floats with the same operations; in fp32 it is not an identity.  Two passes are
 *           supported only with DATA and pad_value == 0, where lo2 = 0 is exact: anything else returns DIAGAN_EUNSUP before any
 *           launch.
 *   bytes   DIAGAN_PIC_BYTES_*.
 * A lane owns four consecutive pixels of one grid row and writes them with 4-byte stores when Wg % 4 == 0 and out is 4-byte
 * aligned, byte by byte otherwise. */
int diagan_pic_grid(const float* x, int B, int C, int H, int W, int nrow, int padding, float pad_value, int norm, double lo,
                    double hi, const float* lohi, int passes, int bytes, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
