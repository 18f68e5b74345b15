/* libdiagan_hip.so -- third header of the C ABI: the PRDC reductions over a block of the pairwise-distance matrix
 * (DESIGN.md section 8k): precision, recall, density and coverage from ONE read of the block.
 *
 * Same conventions and the same prototype grammar as include/diagan_hip.h (this file is read by diagan/_native/prdc_abi.py the way
 * that one is read by diagan/_native): plain C types, device pointers owned by the caller, 0 or a negative DIAGAN_E* code with
 * the text in diagan_last_error(), launch on `stream`, no synchronisation, no allocation.  Every name here starts with
 * diagan_prdc_.
 */
#ifndef DIAGAN_PRDC_H
#define DIAGAN_PRDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace diagan_prdc_reduce needs for a block of rows x cols (0 for a shape it rejects).  Host logic only. */
size_t diagan_prdc_reduce_ws(int rows, int cols);

/* For T[rows][ld] fp32 (diagan.trainer.compute_pr._row_blocks: T[r][c] = |b_c|^2 - 2 a_r.b_c) and d = T[r][c] + row_add[r], in
 * exactly that association (the bits diagan_any_lt_rows / diagan_any_lt_cols compare):
 *   row_min[r]   = min_c d                        fp32  [rows]
 *   row_hit[r]   = any_c d < thr_col[c]           int32 [rows], 0 / 1   (recall's flag: thr_col = radii of the columns' set)
 *   col_hit[c]   = any_r d < thr_row[r]           int32 [cols], 0 / 1   (precision's flag: thr_row = radii of the rows' set)
 *   col_count[c] = #{r : d < thr_row[r]}          int32 [cols]          (density's count)
 * row_add [rows] or NULL (0); thr_col [cols]; thr_row [rows] or NULL: then col_hit and col_count are neither read nor written
 * (and may be NULL).  accumulate != 0: col_hit |= and col_count += what is there, so the row blocks of one matrix can be fed one
 * after the other; the row outputs are always written.  Any rows >= 1, cols >= 1, ld >= cols; T is read once, with 16-byte loads
 * when T and ld * 4 are multiples of 16 and 4-byte loads otherwise.  No atomics: partial results per tile go to ws
 * (ws_bytes >= diagan_prdc_reduce_ws(rows, cols), 16-byte aligned) and a second launch combines them; minimum, OR and integer
 * sums do not depend on the order, so the outputs do not depend on the tiling. */
int diagan_prdc_reduce(const float* T, const float* row_add, const float* thr_col, const float* thr_row, int rows, int cols, int ld,
                       float* row_min, int* row_hit, int* col_hit, int* col_count, int accumulate, void* ws, int64_t ws_bytes,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
