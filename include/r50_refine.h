/*
 * r50_refine.h — C ABI of libr50hip.so, sixth public header: 2D-guided refinement of stitched per-frame pose sequences
 * (INTEGRATION.md section Z).
 *
 * The reference never uses 2D observations at inference, so the stage is this project's definition.  The conventions are those of
 * r50_smooth.h: plain pointers and sizes, 0 on success or a negative r50_status, the text of a refusal through r50_last_error(NULL), every
 * device pointer owned by the caller, launches on `stream`.  Poses are (F, J, 3) fp32 in camera coordinates, 1 <= J <= 64,
 * 1 <= S <= G <= F < 2^31 / 192.  Every argument is checked before any launch (a refused call touches nothing); no atomics, the same bits
 * on every run; each grid is a function of the sizes alone; no workgroup waits for another inside a launch.  The index tables in device
 * memory (seq_start (S+1), row_seq (F), seg_start (G+1), row_seg (F), int32) are trusted: the caller checks them on the host
 * (smooth.DeviceTables builds them; a segment is a maximal run of rows of one sequence with consecutive frame indices).
 *
 * Inputs common to both ops:
 *   x0   (F, J, 3) fp32   the stitched poses; p0 = (double)x0[t][j] and z0 = max(p0_z, z_min) are constants of the fit
 *   rays (F, J, 2) fp32   the 2D observations in normalised image coordinates ((u - cx) / fx, (v - cy) / fy)
 *   conf (F, J) fp32 >= 0 or NULL (all ones); 0 = not detected
 *   edges: 2 E HOST ints (parent, child); E == 0: no bones (edges is not read); else 1 <= E <= J - 1, every index in [0, J),
 *          parent != child, a joint is a child at most once and only in a later edge than the one (if any) of its parent
 *   bone_len (S, E) fp64  the target length of bone e in sequence s
 *
 * The energy, all in fp64, every product and every sum rounded on its own:
 *   E = l2d  sum_{t,j} conf | z0 (X_xy / X_z - ray) |^2       metres^2; a (t, j) with X_z < z_min is skipped
 *     + l3d  sum_{t,j} | X - p0 |^2
 *     + lacc sum_{c : c-1, c, c+1 in one segment} | (X_{c-1} - 2 X_c) + X_{c+1} |^2
 *     + lbone sum_{t,e} ( |X_child - X_parent| - bone_len[seq(t)][e] )^2         a bone of length exactly 0 contributes nothing
 *
 * One sweep is a damped block-Jacobi Gauss-Newton step: every (t, j) is updated from the previous iterate X alone, p = X[t][j]:
 *   term 1, evaluated iff w = l2d * conf != 0 and p_z >= z_min:
 *       s = z0 / p_z, q = p_xy / p_z, r = z0 (q - ray);  g1 = w (s r_x, s r_y, s (-(q_x r_x + q_y r_y)));
 *       H1 = w s^2 [[1, 0, -q_x], [0, 1, -q_y], [-q_x, -q_y, q_x q_x + q_y q_y]]
 *   term 2: g2 = l3d (p - p0), H2 = l3d I
 *   term 3, evaluated iff lacc != 0: over c = t-1, t, t+1 ascending, those with c-1, c, c+1 inside the row's segment, with k_c = 1, -2, 1:
 *       A = sum_c k_c ((X_{c-1} - 2 X_c) + X_{c+1}),  K = sum_c k_c^2;   g3 = lacc A,  H3 = (lacc K) I
 *   term 4, evaluated iff lbone != 0: over the edges that joint j is an endpoint of, in edge-list order, o the other endpoint:
 *       d = p - X[t][o], L = sqrt((d_x^2 + d_y^2) + d_z^2); L == 0: skipped; u = d / L;
 *       B = sum (L - bone_len) u,  U = sum u u^T;   g4 = lbone B,  H4 = lbone U
 *   g = ((g1 + g2) + g3) + g4;  H likewise, the diagonal as (H1 + (l3d + lacc K)) + H4
 *   H = L D L^T without pivoting (l10 = h01 / h00, l20 = h02 / h00, d1 = h11 - l10 h01, l21 = (h12 - l20 h01) / d1,
 *       d2 = h22 - (l20 h02 + l21 (h12 - l20 h01))), forward and back substitution;   p <- p - omega (H^-1 g)
 */
#ifndef R50_REFINE_H_
#define R50_REFINE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* `iters` sweeps from X = x0; out (F, J, 3) fp32 is the last iterate, rounded once.  workspace: 2 F J 3 doubles of device memory, written
 *    before it is read (two fp64 iterates; sweep k reads one and writes the other, the first reads x0, the last writes out).
 *    iters == 0 copies x0 bit for bit; with l2d = lacc = lbone = 0, and for a joint with conf == 0 under lacc = lbone = 0, g is exactly 0
 *    and out holds the bits of x0.  bone_len and edges are read only when lbone != 0 (which needs E >= 1 and bone_len).
 *    Refused unless l3d > 0 (H stays positive definite), l2d, lacc, lbone finite and >= 0, 0 < omega <= 0.75 (the sweep descends iff
 *    2 D / omega - A is positive definite; the second-difference operator has eigenvalues up to 16 lacc against a diagonal of 6 lacc),
 *    z_min > 0 and finite, 0 <= iters <= 1000, the edges valid, and out and workspace overlap neither an input nor each other.
 *    One launch per sweep on `stream`, the next sweep is the next launch: workgroups of 256 over RB = 64 (32 where J > 32) consecutive
 *    rows, the rows and two rows on either side staged in LDS as fp64 ((RB + 4) 3 J doubles: 27,744 bytes at J = 17, 55,296 at J = 64),
 *    every (row, joint) computed by one thread, consecutive threads on consecutive elements.  A stencil never leaves its segment.
 *    No host read and no allocation inside the call. */
int r50_op_pose_fit_sweeps(const float* x0, const float* rays, const float* conf, const int* seg_start, const int* row_seg, const int* row_seq,
                           int64_t F, int G, int S, int J, const int* edges, int E, const double* bone_len, double lambda_2d, double lambda_3d,
                           double lambda_acc, double lambda_bone, double omega, double z_min, int iters, double* workspace, float* out,
                           void* stream);

/* energy (S, 6) fp64, every element written, of the poses x (F, J, 3) fp32, per sequence and NOT multiplied by the weights:
 *    [e2d, e3d, eacc, ebone, the sum of conf over the (t, j) that e2d includes, the number of (t, j) skipped for X_z < z_min].
 *    bone_len == NULL: ebone = 0 (bone_len != NULL needs E >= 1).  One workgroup of 256 per sequence: thread t sums the rows s0 + t,
 *    s0 + t + 256, ... in that order (per row the joints ascending, then the edges), then a fixed tree over the wave and the four waves. */
int r50_op_pose_fit_energy(const float* x, const float* x0, const float* rays, const float* conf, const int* seq_start, const int* row_seg,
                           int64_t F, int S, int J, const int* edges, int E, const double* bone_len, double z_min, double* energy,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R50_REFINE_H_ */
