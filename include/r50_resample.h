/*
 * r50_resample.h — C ABI of libr50hip.so, eighth public header: a pose at any time stamp from the rows around it, for stitched
 * per-frame pose sequences (INTEGRATION.md section AB).
 *
 * The head runs at the cadence it was trained at, and every stage after it inherits that cadence.  The op here resamples a ragged
 * table of pose sequences onto any list of time stamps: the video frames in between, 30 / 60 fps for an animation tool, a uniform
 * clock over a frame index with holes, or the rows a decimated pass left out (`results --dense-holdout`).  The reference animates
 * the poses it has and nothing more, so the stage is this project's definition.  The conventions are those of r50.h: plain pointers
 * and sizes, 0 on success or a negative r50_status, the text of a refusal through r50_last_error(NULL), every device pointer owned
 * by the caller, the launch on `stream`.
 *
 * Inputs
 *   x (F, J, 3) fp32, 1 <= J <= 64, rows of C = 3 J values;  seq_start (S+1) int32 as in r50_smooth.h: sequence s is the rows
 *   a = seq_start[s] .. b-1 = seq_start[s+1]-1;  idx (F) int32 time stamps, STRICTLY INCREASING inside a sequence.
 *   Per output row g of G:  out_time[g] fp64, the time tau;  out_seq[g] int32, the sequence;  out_left[g] int32, the last row i of
 *   that sequence with idx[i] <= tau, or the sequence's first row where tau lies before it.
 *   kind: R50_RESAMPLE_LINEAR or R50_RESAMPLE_CUBIC.  max_gap >= 1.
 *   The four index tables are device memory and trusted, as in r50_smooth.h: the caller checks them on the host
 *   (resample.ResampleTable does) and uploads them.  out_time must be finite.
 *
 * Arithmetic
 *   fp64 on the fp32 positions; every product, quotient and sum is rounded on its own, in the order written (the library is built with
 *   -ffp-contract=off); one rounding to fp32 at the store, and 0.0 is added before it so that no -0 is stored.  A stamp or a difference
 *   of two stamps is converted to fp64 exactly (the difference is formed in 64-bit integers).
 *   An interval [i, i+1] of a sequence is BRIDGED when idx[i+1] - idx[i] <= max_gap, else it is a BREAK.
 *
 * Cases, with i = out_left[g]
 *   tau == idx[i]                        y = x[i], the input's bits; flag 0
 *   tau < idx[a] or tau > idx[b-1]       y = the end row's bits; flag R50_RESAMPLE_OUTSIDE
 *   tau inside a break                   y = the nearer knot's bits, the left one where (tau - idx[i]) <= (idx[i+1] - tau);
 *                                        flag R50_RESAMPLE_IN_BREAK
 *   bridged, linear                      h = idx[i+1] - idx[i], u = (tau - idx[i]) / h:   y = x[i] + u * (x[i+1] - x[i]); flag 0
 *   bridged, cubic                       u2 = u * u, u3 = u2 * u
 *                                        h00 = ((2 * u3) - (3 * u2)) + 1     h10 = (u3 - (2 * u2)) + u
 *                                        h01 = (-(2 * u3)) + (3 * u2)        h11 = u3 - u2
 *                                        y = ((h00 * x[i] + (h10 * h) * m_i) + h01 * x[i+1]) + (h11 * h) * m_{i+1}; flag 0
 *
 * Tangents of the cubic case.  d(p,q) = (x[q] - x[p]) / (idx[q] - idx[p]).  A neighbour of a knot counts only if it is inside the
 * sequence and the interval to it is bridged.  The tangent m_k at knot k:
 *   both neighbours                      hl = idx[k] - idx[k-1], hr = idx[k+1] - idx[k]:
 *                                        m_k = (hr * d(k-1,k) + hl * d(k,k+1)) / (hl + hr)
 *                                        (the three-point parabola's derivative; Catmull-Rom on a uniform clock)
 *   only the right one, and [k+1, k+2] is bridged too:  h0 = idx[k+1] - idx[k], h1 = idx[k+2] - idx[k+1]:
 *                                        m_k = (((2 * h0) + h1) * d(k,k+1) - h0 * d(k+1,k+2)) / (h0 + h1)
 *   only the left one, and [k-2, k-1] is bridged too:   h0 = idx[k] - idx[k-1], h1 = idx[k-1] - idx[k-2]:
 *                                        m_k = (((2 * h0) + h1) * d(k-1,k) - h0 * d(k-2,k-1)) / (h0 + h1)
 *   otherwise (a run of two knots)       the secant d of the interval being evaluated
 * The one-sided three-point rules make the cubic form exact on quadratics in time up to the ends of a run.  An output row reads the
 * rows i-1 .. i+2 of its own sequence and nothing else.
 */
#ifndef R50_RESAMPLE_H_
#define R50_RESAMPLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R50_RESAMPLE_LINEAR 0
#define R50_RESAMPLE_CUBIC 1
#define R50_RESAMPLE_IN_BREAK 1 /* flag bit 0: tau lies strictly inside a break, the nearer knot was copied */
#define R50_RESAMPLE_OUTSIDE 2  /* flag bit 1: tau lies before the first or after the last stamp, the end row was copied */

/* y (G, J, 3) fp32 and flags (G) int32, every element written.  Gather form: one output element per thread, consecutive threads on
 *    consecutive elements of y, so loads and stores are coalesced along the 3 J coordinates.  A workgroup of 256 owns 256 consecutive
 *    elements; the rows they lie in (at most 256 / (3 J) + 2) get their case, u, h and the four Hermite weights formed once, by one
 *    thread each, into LDS (static, under 8 KB); then every thread reads its row's record (the same address across a wave wherever a
 *    wave lies in one row) and the up to four source values of its coordinate.  The grid is ceil(G * 3 J / 256), a function of G and J
 *    alone.  No atomics, no scratch, no host read, no allocation: the same bits on every run.
 *    Refused before any launch: a NULL pointer; F, S, G < 1; S > F; J outside [1, 64]; F or G >= 2^31 / 192; an unknown kind;
 *    max_gap < 1; out_time not 8-byte aligned; y or flags overlapping an input or each other. */
int r50_op_resample_sequences(const float* x, const int* idx, const int* seq_start, int64_t F, int S, int J, const double* out_time,
                              const int* out_seq, const int* out_left, int64_t G, int kind, int max_gap, float* y, int* flags,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R50_RESAMPLE_H_ */
