/*
 * r50_kinematics.h — C ABI of libr50hip.so, fifth public header: joint rotations on a rigid skeleton for per-frame pose sequences
 * (INTEGRATION.md section Y).
 *
 * The reference stops at a matplotlib animation of the joint positions, so the stage is this project's definition.  The conventions are
 * those of r50_smooth.h: plain pointers and sizes, 0 on success or a negative r50_status, the text of a refusal through
 * r50_last_error(NULL), every device pointer owned by the caller, launches on `stream`.  Poses are (F, J, 3) fp32, 1 <= J <= 64,
 * 1 <= S <= F < 2^31 / 192.  Every argument is checked before any launch (a refused call touches nothing); no output may overlap an
 * input or another output; no atomics, the same bits on every run; each grid is a function of the sizes alone.  The index tables in
 * device memory (seq_start, row_seq) are trusted: the caller checks them on the host (smooth.DeviceTables builds them).  The skeleton
 * tables are HOST arrays, checked here.
 *
 * The skeleton.  `edges`: 2 E ints (parent, child), E == J - 1, every index in [0, J), parent != child, a joint is a child at most once
 * and only in a later edge than the one of its parent; the one joint that is nobody's child is the root.  `frames`: 5 NF ints
 * (joint, a0, a1, b0, b1), 0 <= NF <= J, every index in [0, J), a0 != a1, b0 != b1, a joint framed at most once: the joints whose
 * orientation the positions determine in full.  `rest_dirs`: 3 J doubles, a unit vector (| |v|^2 - 1 | <= 1e-12) for every joint but the
 * root, whose entry is not read.  `sign`: 3 doubles, each +1 or -1 with product +1: the positions are multiplied by it on load (the
 * WORLD frame; H36M camera coordinates with y down become y up, left +x, facing +z under (1, -1, -1)); rotations and rest offsets are
 * in the world frame, the rigid positions are stored back in the input's frame (sign flips are exact).
 *
 * The definition, all in fp64 on the fp32 positions, every product and sum rounded on its own (x below is the world-frame pose):
 *   Framed joint j with row (a0, a1, b0, b1):  ex = (x[a1] - x[a0]) / |.|,  ez = (ex X (x[b1] - x[b0])) / |.|,  ey = ez X ex,
 *       R_j = [ex ey ez] as columns; if either norm is exactly 0 the row is DEGENERATE: R_j = R_parent (identity at the root), flag bit 0.
 *   Rest offsets per sequence, rest (S, J, 3) fp64, the root's at 0:
 *       child c of a framed joint p: the mean over the sequence's non-degenerate rows of R_p^T (x_c - x_p);
 *       any other child, and a child of a framed joint with no non-degenerate row: rest_dirs[c] * the mean of |x_c - x_p| over all rows.
 *   Per frame, down the edge list with P[root] = x[root]; for joint j with parent p (R_p = I above the root): P[j] = P[p] + R_p rest[j];
 *       a framed joint gets R_j as above;
 *       a joint with exactly one child c aims at the observed child from the REBUILT joint (position errors do not add up down a limb):
 *           u = R_p rest_dirs[c],  v = (x_c - P[j]) / |.|,  d = u . v,  k = u X v,   R_j = (I + [k]x + [k]x^2 / (1 + d)) R_p
 *           (the minimal rotation: no twist about the bone); |x_c - P[j]| == 0: R_j = R_p, flag bit 1;
 *           1 + d <= 1e-8: R_j = (2 a a^T - I) R_p, flag bit 2, a = (u X e_m) / |.|, e_m the coordinate axis of u's smallest
 *           |component| (the lowest index on a tie);
 *       every other joint (leaves, unframed joints with several children): R_j = R_p.
 *       L_j = R_p^T R_j, L_root = R_root.
 *   Outputs: quat (F, J, 4) fp32 (w, x, y, z) of L_j, Shepperd's largest-pivot form (the trace first, then L00, L11, L22; a later one
 *       only if strictly larger), negated where w < 0;  euler (F, J, 3) fp32 degrees (Z, X, Y) with L = Rz(a) Rx(b) Ry(c):
 *       b = asin(clamp(L21)), a = atan2(-L01, L11), c = atan2(-L20, L22); where |L21| > 1 - 1e-12: c = 0, a = atan2(L10, L00);
 *       (0.0 is added to every quaternion component and angle before it is rounded: there is no -0);
 *       rigid (F, J, 3) fp32: P in the input's frame;  resid (F) fp32: the mean over the joints of |P - x|, rounded once;
 *       flags (F) int32: the OR of the bits above over the frame's joints.
 */
#ifndef R50_KINEMATICS_H_
#define R50_KINEMATICS_H_

#include <stddef.h>
#include <stdint.h>

#ifndef R50_ALIGNED
#define R50_ALIGNED(n)      /* r50.h, "Pointer alignment": the device pointer that follows must be a multiple of n bytes */
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* rest (S, J, 3) fp64, every element written, from x (F, J, 3) fp32 and seq_start (S+1) int32 (sequence s is the rows seq_start[s] ..
 *    seq_start[s+1]-1, at least one).  One workgroup of 256 per sequence: per edge, thread t sums the rows s0 + t, s0 + t + 256, ... in
 *    that order, then a fixed tree over the wave and the four waves; the means are sum / count. */
int r50_op_rest_offsets(const float* x, const int* seq_start, int64_t F, int S, int J, const int* edges, int E, const int* frames, int NF,
                        const double* rest_dirs, const double* sign, double* rest, void* stream);

/* The per-frame pass: x (F, J, 3) fp32, row_seq (F) int32 in [0, S), rest (S, J, 3) fp64 as r50_op_rest_offsets wrote it.
 *    One lane per frame in workgroups of 64 that hold RB = 64 / 32 / 16 / 8 frames for J <= 9 / 18 / 35 / 64.  The rows are staged in
 *    LDS by coalesced loads; the lane's global rotations and rebuilt positions live in LDS as fp64, laid out [joint][lane] with an odd
 *    lane pitch RB + 1 (they are indexed by run-time joint numbers, and a register array so indexed would become scratch); the outputs
 *    are computed from LDS by the whole workgroup, one (frame, joint) per thread, so the stores are coalesced (quat as one 16-byte store
 *    per joint: it must be 16-byte aligned).
 *    LDS budget: 8 (RB + 1) 12 J bytes of fp64 + 4 RB (3 J | 1) bytes of fp32 + 64 bytes of parents <= 64 KiB
 *    (61,536 at J = 64, 60,448 at J = 17). */
int r50_op_pose_rotations(const float* x, const int* row_seq, int64_t F, int S, int J, const int* edges, int E, const int* frames, int NF,
                          const double* rest_dirs, const double* sign, const double* rest, float* R50_ALIGNED(16) quat, float* euler, float* rigid,
                          float* resid, int* flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R50_KINEMATICS_H_ */
