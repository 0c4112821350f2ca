/*
 * r50_multiview.h — C ABI of libr50hip.so, fourth public header: the cameras of one take brought into one frame of reference and fused
 * into one pose per frame.
 *
 * The reference loads camera_wext.pkl per camera and never relates two cameras, so the stage is this project's definition.  The
 * conventions are those of r50_smooth.h: plain pointers and sizes, 0 on success or a negative r50_status, the text of a refusal through
 * r50_last_error(NULL), every device pointer owned by the caller, launches on `stream`.
 *
 * Common to the two ops: poses are (rows, J, 3) fp32, 1 <= J <= 64, 1 <= rows < 2^31 / 192.  Every argument is checked before any
 * launch (a refused call touches nothing); no atomics, the same bits on every run; each grid is a function of the sizes alone.  The
 * index tables in device memory (pair_start, match, peer_start, peer_row, peer_fit) are trusted: the caller checks them on the host
 * (multiview.ViewTable builds them, multiview.DeviceViews checks and uploads them).  fp32 in, fp64 in between; the library is built
 * with -ffp-contract=off, so every product and every sum below is rounded on its own.
 */
#ifndef R50_MULTIVIEW_H_
#define R50_MULTIVIEW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One least-squares rigid fit (rotation and translation, no scale) per pair of views, over the pair's matched rows.
 *    y (rows_y, J, 3), x (rows_x, J, 3) fp32, both read-only; they may be one buffer.  pair_start (P+1) int32: pair p owns the matches
 *    pair_start[p] .. pair_start[p+1]-1; match (M, 2) int32: (row of y, row of x).  fit (P, 16) fp64, every slot written.
 *    Pair p has n = (its matches) * J points; point i is joint i % J of match i / J.  All in fp64:
 *        my, mx   = the centroids of its y and x points
 *        S_uv     = sum (y - my)[u] * (x - mx)[v],   sy = sum |y - my|^2,   sx = sum |x - mx|^2
 *        R        = Horn's quaternion rotation from S: the 4x4 matrix, the cyclic Jacobi with its sweep limit and stop rule, and the
 *                   first-on-ties pick of the largest eigenvalue lambda are those of the protocols' similarity fit (section L)
 *        t        = mx - R my
 *        rms      = sqrt((1/n) sum |R y + t - x|^2), by a third pass over the points (not from sx + sy - 2 lambda, which cancels)
 *    fit[p] = [0..8] R row-major, [9..11] t, [12] n, [13] rms, [14] lambda / sy (the least-squares scale, 0 where sy or sx is 0; a
 *    diagnostic, never applied), [15] sqrt(sx / n).  S = 0 (one point, or no spread) gives R = I; a rank-deficient S still gives an
 *    optimal proper rotation.  A pair without matches gives R = I, t = 0 and zeros.
 *    One workgroup of 256 per pair, three passes (centroids, moments, residual).  The order of every sum: thread t adds its points
 *    i = t, t + 256, t + 512, ... in that order; the 64 lanes of a wave are added by shuffles, v += v[lane + 32], then + 16, 8, 4, 2, 1;
 *    the four waves as ((w0 + w1) + w2) + w3.  Inside a point: (dx*dx + dy*dy) + dz*dz, and R y as ((R0 y0 + R1 y1) + R2 y2) + t. */
int r50_op_view_rigid_fit(const float* y, const float* x, int64_t rows_y, int64_t rows_x, int J, const int* pair_start, const int* match,
                          int P, double* fit, void* stream);

/* Every row fused with its peers, the rows of the other views that show the same frame, in gather form (each output element is written
 * by one thread).
 *    pose, fused (F, J, 3) fp32, fused may not overlap pose; peer_start (F+1) int32: row r's peers are peer_row[peer_start[r] ..
 *    peer_start[r+1]-1] (rows of pose), each mapped into r's camera by the fit peer_fit[...] in [0, P) of fit (P, 16) fp64, the layout
 *    r50_op_view_rigid_fit writes (only slots 0..11 are read).  P >= 0; the kernel reads at most 7 peers of a row, whatever the table says.
 *    The K = 1 + peers contributions of row r, in fp64: c_0 = its own pose, c_k[c] = ((R[c][0] y0 + R[c][1] y1) + R[c][2] y2) + t[c] of
 *    peer k's joint y.  Per coordinate, f =
 *        mode 0  mean:    (((c_0 + c_1) + c_2) + ...) / K
 *        mode 1  median:  the middle of the K values, 0.5 * (a + b) of the two middle ones where K is even (a sorting network)
 *        mode 2  others:  ((c_1 + c_2) + ...) / (K - 1), the peers alone
 *    fused = (float) f, and disagreement[r] = (float) sqrt((1 / (K J)) sum_j sum_k |c_k,j - f_j|^2) over all K contributions (the own
 *    pose included in every mode), per joint k ascending with |d|^2 = (dx*dx + dy*dy) + dz*dz, the joints added over the wave by the
 *    shuffle tree above.  A row without peers: fused holds the bits of pose and disagreement is +0, in every mode.
 *    One wave per row (lane j owns joint j), four rows per workgroup of 256. */
int r50_op_view_fuse(const float* pose, int64_t F, int J, const int* peer_start, const int* peer_row, const int* peer_fit, const double* fit,
                     int P, int mode, float* fused, float* disagreement, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R50_MULTIVIEW_H_ */
