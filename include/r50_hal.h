/*
 * r50_hal.h — C ABI of libr50hip.so, second public header: the hallucinator f_hal of the lifting head.
 *
 * The paper "Predicting 3D Human Dynamics from Video" maps the representation of a single frame to the movie strip f_movie would have
 * produced with temporal context; the reference never builds that module (src/model.py has none), so the stage is this project's
 * definition.  The conventions are those of r50.h: plain pointers and sizes, 0 on success or a negative r50_status, the text of a
 * refusal through r50_last_error(NULL), every device pointer owned by the caller, launches on `stream`.
 */
#ifndef R50_HAL_H_
#define R50_HAL_H_

#include <stddef.h>
#include <stdint.h>

#ifndef R50_ALIGNED
#define R50_ALIGNED(n)      /* r50.h, "Pointer alignment": the device pointer that follows must be a multiple of n bytes */
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* The latent loss of the hallucinator stage and the gradient of f_hal's output, in one pass.
 *    h, phi (rows, d) et elements (0 = bf16, 1 = fp16): f_hal's strips and the teacher's (f_movie's);
 *    dh_reg (rows, d) fp32: the frozen regressor's dX, already times loss_scale;
 *        dh[r, c]    = cast16(dh_reg[r, c] + coef * (h[r, c] - phi[r, c])),   coef = (float)(lambda * 2 / (rows * d) * loss_scale)
 *        loss_lat[0] = mean((h - phi)^2)
 *    per element: dl = h - phi (fp32); the row sum adds dl * dl; the output is dh_reg + coef * dl, no contraction.  row_part: rows
 *    floats of scratch (the per-row sums of squares).  Needs rows >= 1 (within int range), d >= 8 and d % 8 == 0, no null pointer,
 *    h, phi, dh_reg and dh 16-byte aligned, et 0 or 1; checked before any launch (a refused call touches nothing).  Two launches: one
 *    workgroup of 128 per row (16-byte loads and stores, a row touches its own d elements only), then one workgroup adding the rows
 *    in a fixed order.  No atomics: the same bits on every run. */
int r50_op_hal_latent_grad(const void* R50_ALIGNED(16) h, const void* R50_ALIGNED(16) phi, const float* R50_ALIGNED(16) dh_reg, int64_t rows, int d, float lambda, float loss_scale,
                           void* R50_ALIGNED(16) dh, float* loss_lat, float* row_part, int et, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R50_HAL_H_ */
