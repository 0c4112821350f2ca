// Joint rotations on a rigid skeleton for per-frame pose sequences (include/r50_kinematics.h).
// Included after smooth_kernels.h (block_sum_f64).  Everything is fp64 arithmetic on fp32 poses with one rounding at the store; the
// library is built with -ffp-contract=off, so every product and every sum below is rounded on its own.  No atomics anywhere.
//
// The definition (x is the world-frame pose: the input times sign):
//   framed joint j, row (a0, a1, b0, b1): ex = (x[a1] - x[a0]) / |.|, ez = (ex X (x[b1] - x[b0])) / |.|, ey = ez X ex, R_j = [ex ey ez];
//       a norm of exactly 0: R_j = R_parent, flag bit 0.
//   rest[c] per sequence: child of a framed p: the mean over the non-degenerate rows of R_p^T (x_c - x_p); any other child, and a child
//       of a framed joint without such a row: rest_dirs[c] * the mean of |x_c - x_p| over all rows.  The root's is 0.
//   per frame down the edge list: P[root] = x[root], P[j] = P[p] + R_p rest[j]; a framed joint as above; a joint with one child c aims:
//       u = R_p rest_dirs[c], v = (x_c - P[j]) / |.|, d = u . v, k = u X v, R_j = (I + [k]x + [k]x^2 / (1 + d)) R_p;
//       |x_c - P[j]| == 0: R_j = R_p, bit 1;  1 + d <= 1e-8: R_j = (2 a a^T - I) R_p, bit 2, a = (u X e_m) / |.|;  else R_j = R_p.
//   L_j = R_p^T R_j; quat (w, x, y, z) by Shepperd's largest pivot with w >= 0; euler degrees (Z, X, Y), L = Rz Rx Ry; rigid = P in
//       the input's frame; resid = the mean over the joints of |P - x|.
#pragma once

#define KIN_MAX_J 64
#define KIN_INHERIT 0
#define KIN_FRAMED 1
#define KIN_AIM 2

// The skeleton by value in the kernel arguments (checked on the host).  Every index into it below is uniform over the wave, so the
// reads are scalar loads from the argument segment and nothing is copied to scratch.
struct KinSkeleton {
    unsigned char parent[KIN_MAX_J], child[KIN_MAX_J];        // the edges, in order
    unsigned char kind[KIN_MAX_J];                            // per joint: KIN_INHERIT, KIN_FRAMED or KIN_AIM
    unsigned char arg[KIN_MAX_J];                             // per joint: the row of fr (framed) or the one child (aim)
    unsigned char par_of[KIN_MAX_J];                          // per joint: its parent, 255 at the root
    unsigned char fr[KIN_MAX_J][4];                           // a0, a1, b0, b1
    double dirs[KIN_MAX_J][3];
    double sign[3];
    int root;
};

// [ex ey ez] as the columns of r (row-major) from e = x[a1] - x[a0] and f = x[b1] - x[b0]; false where a norm is exactly 0.
__device__ inline bool kin_frame(double e0, double e1, double e2, double f0, double f1, double f2, double* r) {
    const double n1 = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    if (n1 == 0.0) return false;
    e0 /= n1;
    e1 /= n1;
    e2 /= n1;
    double z0 = e1 * f2 - e2 * f1, z1 = e2 * f0 - e0 * f2, z2 = e0 * f1 - e1 * f0;
    const double n2 = sqrt((z0 * z0 + z1 * z1) + z2 * z2);
    if (n2 == 0.0) return false;
    z0 /= n2;
    z1 /= n2;
    z2 /= n2;
    r[0] = e0, r[3] = e1, r[6] = e2;
    r[1] = z1 * e2 - z2 * e1, r[4] = z2 * e0 - z0 * e2, r[7] = z0 * e1 - z1 * e0;
    r[2] = z0, r[5] = z1, r[8] = z2;
    return true;
}

// One workgroup of 256 per sequence; per edge one pass over the sequence's rows, thread t taking the rows s0 + t, s0 + t + 256, ... in
// that order, then block_sum_f64's fixed tree per sum.  The branch on the parent's kind is uniform over the workgroup.
__global__ __launch_bounds__(256) void rest_offsets_kernel(const float* __restrict__ x, const int* __restrict__ seq_start, int J,
                                                           KinSkeleton sk, double* __restrict__ rest) {
    __shared__ double red[4];
    const int s = blockIdx.x, tid = threadIdx.x, C = 3 * J;
    const int s0 = seq_start[s], n = seq_start[s + 1] - s0;
    const double g0 = sk.sign[0], g1 = sk.sign[1], g2 = sk.sign[2];
    double* __restrict__ dst = rest + (size_t)s * C;
    if (tid < 3) dst[3 * sk.root + tid] = 0.0;
    for (int b = 0; b < J - 1; ++b) {
        const int pa = sk.parent[b], ch = sk.child[b];
        const bool framed = sk.kind[pa] == KIN_FRAMED;
        const int fi = sk.arg[pa];
        const int a0 = sk.fr[fi][0], a1 = sk.fr[fi][1], b0 = sk.fr[fi][2], b1 = sk.fr[fi][3];
        double len = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0, cnt = 0.0;
        for (int r = tid; r < n; r += 256) {
            const float* __restrict__ row = x + (size_t)(s0 + r) * C;
            const double d0 = g0 * (double)row[3 * ch] - g0 * (double)row[3 * pa];
            const double d1 = g1 * (double)row[3 * ch + 1] - g1 * (double)row[3 * pa + 1];
            const double d2 = g2 * (double)row[3 * ch + 2] - g2 * (double)row[3 * pa + 2];
            len += sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            if (framed) {
                double m[9];
                if (kin_frame(g0 * (double)row[3 * a1] - g0 * (double)row[3 * a0], g1 * (double)row[3 * a1 + 1] - g1 * (double)row[3 * a0 + 1],
                              g2 * (double)row[3 * a1 + 2] - g2 * (double)row[3 * a0 + 2], g0 * (double)row[3 * b1] - g0 * (double)row[3 * b0],
                              g1 * (double)row[3 * b1 + 1] - g1 * (double)row[3 * b0 + 1],
                              g2 * (double)row[3 * b1 + 2] - g2 * (double)row[3 * b0 + 2], m)) {
                    v0 += (m[0] * d0 + m[3] * d1) + m[6] * d2;
                    v1 += (m[1] * d0 + m[4] * d1) + m[7] * d2;
                    v2 += (m[2] * d0 + m[5] * d1) + m[8] * d2;
                    cnt += 1.0;
                }
            }
        }
        const double mean_len = block_sum_f64(len, red) / (double)n;
        double o0 = sk.dirs[ch][0] * mean_len, o1 = sk.dirs[ch][1] * mean_len, o2 = sk.dirs[ch][2] * mean_len;
        if (framed) {
            const double c = block_sum_f64(cnt, red);
            v0 = block_sum_f64(v0, red);
            v1 = block_sum_f64(v1, red);
            v2 = block_sum_f64(v2, red);
            if (c > 0.0) o0 = v0 / c, o1 = v1 / c, o2 = v2 / c;
        }
        if (tid == 0) dst[3 * ch] = o0, dst[3 * ch + 1] = o1, dst[3 * ch + 2] = o2;
    }
}

__host__ __device__ inline int pose_rot_rows(int J) { return J <= 9 ? 64 : J <= 18 ? 32 : J <= 35 ? 16 : 8; }   // frames per workgroup
__host__ __device__ inline int pose_rot_pitch(int C) { return C | 1; }                                          // odd: lanes on distinct banks
__host__ __device__ inline size_t pose_rot_lds(int J) {
    const int rb = pose_rot_rows(J);
    return (size_t)(rb + 1) * 12 * J * sizeof(double) + (size_t)rb * pose_rot_pitch(3 * J) * sizeof(float) + KIN_MAX_J;
}

// (w, x, y, z) of the rotation l (row-major): Shepperd's form on the largest of the trace, l00, l11, l22 (a later one only if strictly
// larger), negated where w < 0.
__device__ inline void kin_quat(const double* l, double* q) {
    const double t = (l[0] + l[4]) + l[8];
    int pick = 0;
    double best = t;
    if (l[0] > best) best = l[0], pick = 1;
    if (l[4] > best) best = l[4], pick = 2;
    if (l[8] > best) pick = 3;
    double w, a, b, c;
    if (pick == 0) {
        w = 0.5 * sqrt(1.0 + t);
        const double f = 4.0 * w;
        a = (l[7] - l[5]) / f, b = (l[2] - l[6]) / f, c = (l[3] - l[1]) / f;
    } else if (pick == 1) {
        a = 0.5 * sqrt(((1.0 + l[0]) - l[4]) - l[8]);
        const double f = 4.0 * a;
        w = (l[7] - l[5]) / f, b = (l[1] + l[3]) / f, c = (l[2] + l[6]) / f;
    } else if (pick == 2) {
        b = 0.5 * sqrt(((1.0 + l[4]) - l[0]) - l[8]);
        const double f = 4.0 * b;
        w = (l[2] - l[6]) / f, a = (l[1] + l[3]) / f, c = (l[5] + l[7]) / f;
    } else {
        c = 0.5 * sqrt(((1.0 + l[8]) - l[0]) - l[4]);
        const double f = 4.0 * c;
        w = (l[3] - l[1]) / f, a = (l[2] + l[6]) / f, b = (l[5] + l[7]) / f;
    }
    if (w < 0.0) w = -w, a = -a, b = -b, c = -c;
    q[0] = w + 0.0, q[1] = a + 0.0, q[2] = b + 0.0, q[3] = c + 0.0;                 // + 0.0: a -0 becomes +0
}

// Degrees (Z, X, Y) with l = Rz(z) Rx(x) Ry(y); the + 0.0 turns a -0 into +0.
__device__ inline void kin_euler(const double* l, double* e) {
    const double deg = 57.29577951308232;
    const double s = l[7] > 1.0 ? 1.0 : l[7] < -1.0 ? -1.0 : l[7];
    double z, y;
    if (fabs(l[7]) > 1.0 - 1e-12) {
        y = 0.0;
        z = atan2(l[3], l[0]);
    } else {
        z = atan2(-l[1], l[4]);
        y = atan2(-l[6], l[8]);
    }
    e[0] = z * deg + 0.0, e[1] = asin(s) * deg + 0.0, e[2] = y * deg + 0.0;
}

// RB frames per workgroup of 64.  LDS: rs[(9 j + k) * RP + lane] the global rotations and ps[(3 j + k) * RP + lane] the rebuilt
// positions (fp64, RP = RB + 1 odd, so that both the walk, lane = frame, and the output pass, lane = joint at a pitch of 9 RP or 3 RP,
// find distinct banks); xs the input rows as fp32, row-major with an odd pitch; par the parents.  Lane l < rows walks the edge list of
// frame r0 + l; then the workgroup computes and stores the outputs of the (frame, joint) pairs in memory order.
__global__ __launch_bounds__(64) void pose_rotations_kernel(const float* __restrict__ x, const int* __restrict__ row_seq, int F, int J,
                                                            KinSkeleton sk, const double* __restrict__ rest, float* __restrict__ quat,
                                                            float* __restrict__ euler, float* __restrict__ rigid,
                                                            float* __restrict__ resid, int* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kin_sm[];
    const int C = 3 * J, RB = pose_rot_rows(J), RP = RB + 1, XP = pose_rot_pitch(C);
    double* rs = reinterpret_cast<double*>(kin_sm);
    double* ps = rs + (size_t)9 * J * RP;
    float* xs = reinterpret_cast<float*>(ps + (size_t)3 * J * RP);
    unsigned char* par = reinterpret_cast<unsigned char*>(xs + (size_t)RB * XP);
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * RB;
    const int rows = F - r0 < RB ? F - r0 : RB;
    const float* __restrict__ src = x + (size_t)r0 * C;
    for (int i = tid; i < rows * C; i += 64) {
        const int l = i / C;
        xs[l * XP + (i - l * C)] = src[i];
    }
    for (int j = 0; j < J; ++j)
        if (tid == 0) par[j] = sk.par_of[j];
    __syncthreads();
    const double g0 = sk.sign[0], g1 = sk.sign[1], g2 = sk.sign[2];
    if (tid < rows) {
        const float* row = xs + tid * XP;
        const double* __restrict__ off = rest + (size_t)row_seq[r0 + tid] * C;
        int flag = 0;
        for (int b = -1; b < J - 1; ++b) {
            const int j = b < 0 ? sk.root : sk.child[b];
            double rp[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
            double p0, p1, p2;
            if (b < 0) {
                p0 = g0 * (double)row[3 * j], p1 = g1 * (double)row[3 * j + 1], p2 = g2 * (double)row[3 * j + 2];
            } else {
                const int pa = sk.parent[b];
#pragma unroll
                for (int k = 0; k < 9; ++k) rp[k] = rs[(9 * pa + k) * RP + tid];
                const double o0 = off[3 * j], o1 = off[3 * j + 1], o2 = off[3 * j + 2];
                p0 = ps[(3 * pa) * RP + tid] + ((rp[0] * o0 + rp[1] * o1) + rp[2] * o2);
                p1 = ps[(3 * pa + 1) * RP + tid] + ((rp[3] * o0 + rp[4] * o1) + rp[5] * o2);
                p2 = ps[(3 * pa + 2) * RP + tid] + ((rp[6] * o0 + rp[7] * o1) + rp[8] * o2);
            }
            ps[(3 * j) * RP + tid] = p0, ps[(3 * j + 1) * RP + tid] = p1, ps[(3 * j + 2) * RP + tid] = p2;
            double rj[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) rj[k] = rp[k];
            const int kind = sk.kind[j];
            if (kind == KIN_FRAMED) {
                const int fi = sk.arg[j];
                const int a0 = sk.fr[fi][0], a1 = sk.fr[fi][1], b0 = sk.fr[fi][2], b1 = sk.fr[fi][3];
                double m[9];
                if (kin_frame(g0 * (double)row[3 * a1] - g0 * (double)row[3 * a0], g1 * (double)row[3 * a1 + 1] - g1 * (double)row[3 * a0 + 1],
                              g2 * (double)row[3 * a1 + 2] - g2 * (double)row[3 * a0 + 2], g0 * (double)row[3 * b1] - g0 * (double)row[3 * b0],
                              g1 * (double)row[3 * b1 + 1] - g1 * (double)row[3 * b0 + 1],
                              g2 * (double)row[3 * b1 + 2] - g2 * (double)row[3 * b0 + 2], m)) {
#pragma unroll
                    for (int k = 0; k < 9; ++k) rj[k] = m[k];
                } else {
                    flag |= 1;
                }
            } else if (kind == KIN_AIM) {
                const int c = sk.arg[j];
                const double t0 = sk.dirs[c][0], t1 = sk.dirs[c][1], t2 = sk.dirs[c][2];
                const double u0 = (rp[0] * t0 + rp[1] * t1) + rp[2] * t2;
                const double u1 = (rp[3] * t0 + rp[4] * t1) + rp[5] * t2;
                const double u2 = (rp[6] * t0 + rp[7] * t1) + rp[8] * t2;
                double v0 = g0 * (double)row[3 * c] - p0, v1 = g1 * (double)row[3 * c + 1] - p1, v2 = g2 * (double)row[3 * c + 2] - p2;
                const double nv = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
                if (nv == 0.0) {
                    flag |= 2;
                } else {
                    v0 /= nv;
                    v1 /= nv;
                    v2 /= nv;
                    const double d1 = 1.0 + ((u0 * v0 + u1 * v1) + u2 * v2);
                    double a[9];                                                       // the rotation applied on the left of R_p
                    if (d1 <= 1e-8) {
                        flag |= 4;
                        const double m0 = fabs(u0), m1 = fabs(u1), m2 = fabs(u2);
                        const int ax = (m0 <= m1 && m0 <= m2) ? 0 : (m1 <= m2 ? 1 : 2);
                        const double e0 = ax == 0 ? 1.0 : 0.0, e1 = ax == 1 ? 1.0 : 0.0, e2 = ax == 2 ? 1.0 : 0.0;
                        double w0 = u1 * e2 - u2 * e1, w1 = u2 * e0 - u0 * e2, w2 = u0 * e1 - u1 * e0;
                        const double nw = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
                        w0 /= nw;
                        w1 /= nw;
                        w2 /= nw;
                        a[0] = 2.0 * (w0 * w0) - 1.0, a[1] = 2.0 * (w0 * w1), a[2] = 2.0 * (w0 * w2);
                        a[3] = 2.0 * (w1 * w0), a[4] = 2.0 * (w1 * w1) - 1.0, a[5] = 2.0 * (w1 * w2);
                        a[6] = 2.0 * (w2 * w0), a[7] = 2.0 * (w2 * w1), a[8] = 2.0 * (w2 * w2) - 1.0;
                    } else {
                        const double k0 = u1 * v2 - u2 * v1, k1 = u2 * v0 - u0 * v2, k2 = u0 * v1 - u1 * v0;
                        // [k]x^2 = k k^T - |k|^2 I
                        const double kk = (k0 * k0 + k1 * k1) + k2 * k2;
                        a[0] = 1.0 + (k0 * k0 - kk) / d1, a[1] = -k2 + (k0 * k1) / d1, a[2] = k1 + (k0 * k2) / d1;
                        a[3] = k2 + (k1 * k0) / d1, a[4] = 1.0 + (k1 * k1 - kk) / d1, a[5] = -k0 + (k1 * k2) / d1;
                        a[6] = -k1 + (k2 * k0) / d1, a[7] = k0 + (k2 * k1) / d1, a[8] = 1.0 + (k2 * k2 - kk) / d1;
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int k = 0; k < 3; ++k) rj[3 * i + k] = (a[3 * i] * rp[k] + a[3 * i + 1] * rp[3 + k]) + a[3 * i + 2] * rp[6 + k];
                }
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) rs[(9 * j + k) * RP + tid] = rj[k];
        }
        double acc = 0.0;
        for (int j = 0; j < J; ++j) {
            const double d0 = ps[(3 * j) * RP + tid] - g0 * (double)row[3 * j];
            const double d1 = ps[(3 * j + 1) * RP + tid] - g1 * (double)row[3 * j + 1];
            const double d2 = ps[(3 * j + 2) * RP + tid] - g2 * (double)row[3 * j + 2];
            acc += sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        }
        resid[r0 + tid] = (float)(acc / (double)J);
        flags[r0 + tid] = flag;
    }
    __syncthreads();
    float* __restrict__ dst = rigid + (size_t)r0 * C;
    for (int i = tid; i < rows * C; i += 64) {
        const int l = i / C, jc = i - l * C;
        const int k = jc % 3;
        dst[i] = (float)((k == 0 ? g0 : k == 1 ? g1 : g2) * ps[jc * RP + l]);
    }
    float4* __restrict__ qd = reinterpret_cast<float4*>(quat) + (size_t)r0 * J;
    float* __restrict__ ed = euler + (size_t)r0 * C;
    for (int i = tid; i < rows * J; i += 64) {
        const int l = i / J, j = i - l * J;
        const int pa = par[j];
        double rj[9], lo[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) rj[k] = rs[(9 * j + k) * RP + l];
        if (pa == 255) {
#pragma unroll
            for (int k = 0; k < 9; ++k) lo[k] = rj[k];
        } else {
            double rp[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) rp[k] = rs[(9 * pa + k) * RP + l];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int k = 0; k < 3; ++k) lo[3 * a + k] = (rp[a] * rj[k] + rp[3 + a] * rj[3 + k]) + rp[6 + a] * rj[6 + k];
        }
        double q[4], e[3];
        kin_quat(lo, q);
        kin_euler(lo, e);
        qd[i] = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
        ed[3 * i] = (float)e[0], ed[3 * i + 1] = (float)e[1], ed[3 * i + 2] = (float)e[2];
    }
}
