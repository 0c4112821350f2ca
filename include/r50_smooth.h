/*
 * r50_smooth.h — C ABI of libr50hip.so, third public header: temporal smoothing and constant bone lengths for stitched per-frame
 * pose sequences.
 *
 * The reference animates the raw poses (src/visualize_2d.py) and has no such step, so the stage is this project's definition.  The
 * conventions are those of r50.h: plain pointers and sizes, 0 on success or a negative r50_status, the text of a refusal through
 * r50_last_error(NULL), every device pointer owned by the caller, launches on `stream`.
 *
 * Common to the four ops: poses are (F, J, 3) fp32 rows of C = 3 J values, 1 <= J <= 64, 1 <= F < 2^31 / 192.  Every argument is
 * checked before any launch (a refused call touches nothing); `out` may not overlap `x`; no atomics, the same bits on every run; each
 * grid is a function of the sizes alone.  The index tables in device memory (seg_start, row_seg, seq_start, row_seq) are trusted: the
 * caller checks them on the host (smooth.segment_table builds them).  `edges` is a HOST array of 2 E ints (parent, child), checked here.
 */
#ifndef R50_SMOOTH_H_
#define R50_SMOOTH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A position-dependent FIR filter over the segments of a ragged table, in gather form (each output element is written by one thread).
 *    x, out (F, J, 3) fp32; seg_start (G+1) int32: segment g is the rows seg_start[g] .. seg_start[g+1]-1; row_seg (F) int32: a row's
 *    segment; coef (W, W) fp64 in device memory, W odd, 1 <= W <= 63, R = (W - 1) / 2.
 *    For the row at position pos of a segment of L >= W rows:   lo = clamp(pos - R, 0, L - W),  e = pos - lo,
 *        out = (float) sum_k coef[e][k] * (double)x[lo + k]      k ascending, every product and every sum rounded on its own (fp64)
 *    The rows of a segment with L < W are copied bit for bit.  short_rows (2) int32 is written in full: [0] = the number of copied rows,
 *    [1] = the number of segments they lie in (integer sums over the G segments in a fixed tree, by workgroup 0).
 *    One workgroup of 256 per 64 consecutive rows; the table sits in LDS as fp64 (W * W * 8 bytes, 31,752 at W = 63); a window never
 *    leaves its segment, so x is read inside [0, F) only. */
int r50_op_fir_sequences(const float* x, const int* seg_start, const int* row_seg, int64_t F, int G, int J, const double* coef, int W,
                         float* out, int* short_rows, void* stream);

/* The One-Euro filter (Casiez, Roussel and Vogel 2012) per coordinate over the segments seg_start (G+1) of x (F, J, 3) fp32, where
 *    F = seg_start[G] is given as well.  Causal; the state restarts at every segment's first row, which is copied bit for bit.  With
 *    te = 1 / rate and alpha(fc) = 1 / (1 + 1 / (((2 pi) * fc) * te)), in fp64, for t >= 1:
 *        dx    = (x_t - xhat_{t-1}) * rate
 *        dxhat = dxhat + alpha(d_cutoff) * (dx - dxhat)                  dxhat = 0 at the first row
 *        fc    = min_cutoff + beta * |dxhat|
 *        xhat  = xhat + alpha(fc) * (x_t - xhat)                         out_t = (float) xhat
 *    Needs rate, min_cutoff, d_cutoff > 0 and beta >= 0, all finite.  One wave per (segment, 64 coordinates), four waves a workgroup;
 *    the loads run four rows ahead of the recurrence. */
int r50_op_one_euro_sequences(const float* x, const int* seg_start, int64_t F, int G, int J, double rate, double min_cutoff, double beta,
                              double d_cutoff, float* out, void* stream);

/* Bone-length statistics per (sequence, edge): x (F, J, 3) fp32, seq_start (S+1) int32 (sequence s is the rows seq_start[s] ..
 *    seq_start[s+1]-1, n_s >= 1 of them), edges: 2 E host ints (parent, child), 1 <= E <= J - 1, every index in [0, J), parent != child,
 *    a joint is a child at most once and only in a later edge than the one (if any) of its parent.
 *        stats[s][b][0] = mean over the rows of len = sqrt((dx*dx + dy*dy) + dz*dz), d = (double)child - (double)parent
 *        stats[s][b][1] = sum over the rows of (len - mean)^2
 *    stats (S, E, 2) fp64, every element written.  One workgroup of 256 per sequence: per-thread partial sums in row order, then a fixed
 *    tree over the wave and the four waves. */
int r50_op_bone_stats(const float* x, const int* seq_start, int64_t F, int S, int J, const int* edges, int E, double* stats, void* stream);

/* Every frame rebuilt with the bone lengths stats[row_seq[r]][b][0], down the edge list:
 *        child' = parent' + (len_b * d) / |d|,   d = (double)child - (double)parent of x;   child' = parent' + d  where |d| == 0
 *    parent' is the fp64 value from earlier in the list (a joint that is no edge's child keeps its bits); only the store rounds to fp32.
 *    x, out (F, J, 3) fp32, row_seq (F) int32 in [0, S), stats (S, E, 2) fp64 as r50_op_bone_stats wrote it; edges as there.
 *    One lane per row, 64 rows (16 where J > 28) per workgroup of 64, rows staged through LDS so that loads and stores are coalesced. */
int r50_op_bone_rebuild(const float* x, const int* row_seq, int64_t F, int S, int J, const int* edges, int E, const double* stats, float* out,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R50_SMOOTH_H_ */
