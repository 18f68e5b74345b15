/* libdiagan_hip.so -- the resident-image form of the split-operand lone-tile GEMM (tile_cfg 16, csrc/conv_gemm_x3.hip).
 *
 * Same conventions and the same prototype grammar as include/diagan_hip.h (read by diagan/_native/conv_x3_abi.py the way that header is
 * read by diagan/_native).  The entry points live in a header of their own, like the dataset feed's in include/diagan_data.h: the table of
 * include/diagan_hip.h is pinned name by name by tests/test_native_abi.py.
 *
 * Where a 64-row tile of a tile_cfg 16 launch is one whole 8 x 8 image -- the 3 x 3 / stride 1 / pad 1 convolutions and data gradients of
 * SNGAN-32's discriminator blocks 3 and 4, Ci <= 128 -- the kernel stages that image ONCE, as three bf16 piece planes of a 10 x 10 zero-
 * bordered image in LDS, and reads the A-fragments of the nine taps from it; the per-tap form loads, splits and writes the same pixels
 * nine times.  Same K-steps, same accumulation order: the two forms' results are bit-identical.  Every other tile_cfg 16 launch keeps
 * the per-tap form whatever the switch says.
 */
#ifndef DIAGAN_CONV_X3_H
#define DIAGAN_CONV_X3_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mode 1 / 0 / -1: the resident form where the geometry qualifies / never / DIAGAN_GEMM_X3_RESIDENT (process-wide: diagnostics and the
 * tests' like-with-like runs; a caller that wants one launch another way sets diagan_conv_opts.gemm_x3_resident for that call). */
int diagan_conv_gemm_set_x3_resident(int mode);
int diagan_conv_gemm_get_x3_resident(void);
/* The form the last tile_cfg 16 launch of the calling thread ran: 1 per-tap, 2 resident image; 0 before the first. */
int diagan_conv_gemm_last_x3_form(void);
/* 1 when a diagan_conv_gemm launch of this geometry (arguments as there) qualifies for the resident form: what tile_cfg 16 asks, and
 * R = S = 3, (dr, off) = (1, -1) or (-1, 1), Hi = Wi = Ho = Wo = 8, and a Ci whose LDS image fits beside the weight stages (<= 128). */
int diagan_conv_gemm_x3_resident_ok(int B, int Hi, int Wi, int Ci, int Ho, int Wo, int Co, int R, int S, int sy, int dr, int off, int up,
                                    int Kp, int pro_mode);

#ifdef __cplusplus
}
#endif
#endif
