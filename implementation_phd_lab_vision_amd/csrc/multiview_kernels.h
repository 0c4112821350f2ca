// The cameras of one take brought into one frame of reference and fused (include/r50_multiview.h).
// Included after kernels.h (jacobi4_rotate, POSE_JACOBI_SWEEPS, wave_sum_f64).  Everything is fp64 arithmetic on fp32 poses with one
// rounding at the store; the library is built with -ffp-contract=off, so every product and every sum below is rounded on its own.
// No atomics anywhere.
#pragma once

#define VIEW_MAX_J 64
#define VIEW_MAX_PEERS 7                                                        // peers of a row the fuse kernel reads: 8 views at most
#define VIEW_FIT_SLOTS 16

// Horn's quaternion rotation from S_uv = sum Y0[u] X0[v]: r = the proper rotation that maximises sum X0 . r Y0, lam = that maximum (the
// largest eigenvalue of N(S)).  The matrix, the sweeps, the stop rule and the first-on-ties pick are pose_similarity_fit's (kernels.h).
// S = 0 leaves the eigenvectors at the identity and picks the first: q = (1, 0, 0, 0), r = I.
__host__ __device__ inline void horn_rotation_from_s(const double (&s)[3][3], double (&r)[3][3], double& lam) {
    double n[4][4] = {{s[0][0] + s[1][1] + s[2][2], s[1][2] - s[2][1], s[2][0] - s[0][2], s[0][1] - s[1][0]},
                      {s[1][2] - s[2][1], s[0][0] - s[1][1] - s[2][2], s[0][1] + s[1][0], s[2][0] + s[0][2]},
                      {s[2][0] - s[0][2], s[0][1] + s[1][0], -s[0][0] + s[1][1] - s[2][2], s[1][2] + s[2][1]},
                      {s[0][1] - s[1][0], s[2][0] + s[0][2], s[1][2] + s[2][1], -s[0][0] - s[1][1] + s[2][2]}};
    double ev[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
    double fro2 = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) fro2 += n[u][v] * n[u][v];
    for (int sweep = 0; sweep < POSE_JACOBI_SWEEPS; ++sweep) {
        const double off = n[0][1] * n[0][1] + n[0][2] * n[0][2] + n[0][3] * n[0][3] + n[1][2] * n[1][2] + n[1][3] * n[1][3] +
                           n[2][3] * n[2][3];
        if (off <= 1e-34 * fro2) break;
        jacobi4_rotate<0, 1>(n, ev);
        jacobi4_rotate<0, 2>(n, ev);
        jacobi4_rotate<0, 3>(n, ev);
        jacobi4_rotate<1, 2>(n, ev);
        jacobi4_rotate<1, 3>(n, ev);
        jacobi4_rotate<2, 3>(n, ev);
    }
    lam = n[0][0];
    double q[4] = {ev[0][0], ev[1][0], ev[2][0], ev[3][0]};                      // the largest eigenvalue (first on ties)
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        if (n[i][i] > lam) {
            lam = n[i][i];
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = ev[u][i];
        }
    }
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] /= qn;
    const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
    r[0][0] = w * w + qx * qx - qy * qy - qz * qz; r[0][1] = 2.0 * (qx * qy - w * qz); r[0][2] = 2.0 * (qx * qz + w * qy);
    r[1][0] = 2.0 * (qx * qy + w * qz); r[1][1] = w * w - qx * qx + qy * qy - qz * qz; r[1][2] = 2.0 * (qy * qz - w * qx);
    r[2][0] = 2.0 * (qx * qz - w * qy); r[2][1] = 2.0 * (qy * qz + w * qx); r[2][2] = w * w - qx * qx - qy * qy + qz * qz;
}

// The sums of v[0..N) over the 256 threads in a fixed tree (wave, then ((w0 + w1) + w2) + w3), returned to every thread; red: 4 N doubles.
template <int N>
__device__ inline void block_sum_vec_f64(double (&v)[N], double* red) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = wave_sum_f64(v[q]);
    __syncthreads();                                                            // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) red[(threadIdx.x >> 6) * N + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = ((red[q] + red[N + q]) + red[2 * N + q]) + red[3 * N + q];
}

// c[.] = ((r[c][0] y0 + r[c][1] y1) + r[c][2] y2) + t[c] with f = [r row-major (9), t (3)].
__device__ inline void view_transform(const double* __restrict__ f, double y0, double y1, double y2, double (&c)[3]) {
#pragma unroll
    for (int u = 0; u < 3; ++u) c[u] = ((f[3 * u] * y0 + f[3 * u + 1] * y1) + f[3 * u + 2] * y2) + f[9 + u];
}

// One workgroup per pair; three passes over the pair's n = matches * J points, thread t taking the points t, t + 256, ... in that order
// (point i = joint i % J of match i / J).  A latency-tolerant fp64 reduction: ~100 points per thread and pass at 1,500 rows of 17 joints.
// Thread 0 alone solves the 4x4 eigenproblem and hands r and t to the others through LDS.
__global__ __launch_bounds__(256) void view_rigid_fit_kernel(const float* __restrict__ y, const float* __restrict__ x, int J,
                                                             const int* __restrict__ pair_start, const int* __restrict__ match,
                                                             double* __restrict__ fit) {
    __shared__ double red[4 * 11];
    __shared__ double rt[12];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int m0 = pair_start[p], rows = pair_start[p + 1] - m0;
    double* __restrict__ out = fit + (size_t)p * VIEW_FIT_SLOTS;
    if (rows < 1) {                                                             // no match: the identity and zeros
        if (tid < VIEW_FIT_SLOTS) out[tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.0 : 0.0;
        return;
    }
    const int n = rows * J;
    const int* __restrict__ mt = match + (size_t)m0 * 2;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += 256) {
        const int m = i / J, j = i - m * J;
        const float* __restrict__ py = y + ((size_t)mt[2 * (size_t)m] * J + j) * 3;
        const float* __restrict__ px = x + ((size_t)mt[2 * (size_t)m + 1] * J + j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[c] += (double)py[c];
            a[3 + c] += (double)px[c];
        }
    }
    block_sum_vec_f64<6>(a, red);
    const double my[3] = {a[0] / (double)n, a[1] / (double)n, a[2] / (double)n};
    const double mx[3] = {a[3] / (double)n, a[4] / (double)n, a[5] / (double)n};
    double b[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};        // S row-major, sy, sx
    for (int i = tid; i < n; i += 256) {
        const int m = i / J, j = i - m * J;
        const float* __restrict__ py = y + ((size_t)mt[2 * (size_t)m] * J + j) * 3;
        const float* __restrict__ px = x + ((size_t)mt[2 * (size_t)m + 1] * J + j) * 3;
        const double y0[3] = {(double)py[0] - my[0], (double)py[1] - my[1], (double)py[2] - my[2]};
        const double x0[3] = {(double)px[0] - mx[0], (double)px[1] - mx[1], (double)px[2] - mx[2]};
        b[9] += (y0[0] * y0[0] + y0[1] * y0[1]) + y0[2] * y0[2];
        b[10] += (x0[0] * x0[0] + x0[1] * x0[1]) + x0[2] * x0[2];
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) b[3 * u + v] += y0[u] * x0[v];
    }
    block_sum_vec_f64<11>(b, red);
    if (tid == 0) {
        const double s[3][3] = {{b[0], b[1], b[2]}, {b[3], b[4], b[5]}, {b[6], b[7], b[8]}};
        double r[3][3], lam;
        horn_rotation_from_s(s, r, lam);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
#pragma unroll
            for (int v = 0; v < 3; ++v) rt[3 * u + v] = r[u][v];
            rt[9 + u] = mx[u] - ((r[u][0] * my[0] + r[u][1] * my[1]) + r[u][2] * my[2]);
        }
#pragma unroll
        for (int q = 0; q < 12; ++q) out[q] = rt[q];
        out[12] = (double)n;
        out[14] = (b[9] > 0.0 && b[10] > 0.0) ? lam / b[9] : 0.0;
        out[15] = sqrt(b[10] / (double)n);
    }
    __syncthreads();
    double e[1] = {0.0};
    for (int i = tid; i < n; i += 256) {
        const int m = i / J, j = i - m * J;
        const float* __restrict__ py = y + ((size_t)mt[2 * (size_t)m] * J + j) * 3;
        const float* __restrict__ px = x + ((size_t)mt[2 * (size_t)m + 1] * J + j) * 3;
        double c[3];
        view_transform(rt, (double)py[0], (double)py[1], (double)py[2], c);
        const double d0 = c[0] - (double)px[0], d1 = c[1] - (double)px[1], d2 = c[2] - (double)px[2];
        e[0] += (d0 * d0 + d1 * d1) + d2 * d2;
    }
    block_sum_vec_f64<1>(e, red);
    if (tid == 0) out[13] = sqrt(e[0] / (double)n);
}

__device__ inline void view_cswap(double& a, double& b) {
    const double lo = b < a ? b : a, hi = b < a ? a : b;
    a = lo;
    b = hi;
}

// The median of v[0..K), 1 <= K <= 8, with v[K..8) = +inf: the 19-exchange sorting network of 8, then the middle value, or half the sum
// of the two middle ones where K is even.  Every index is a constant, so v stays in registers.
__device__ inline double view_median8(double (&v)[8], int K) {
    view_cswap(v[0], v[1]); view_cswap(v[2], v[3]); view_cswap(v[4], v[5]); view_cswap(v[6], v[7]);
    view_cswap(v[0], v[2]); view_cswap(v[1], v[3]); view_cswap(v[4], v[6]); view_cswap(v[5], v[7]);
    view_cswap(v[1], v[2]); view_cswap(v[5], v[6]); view_cswap(v[0], v[4]); view_cswap(v[3], v[7]);
    view_cswap(v[1], v[5]); view_cswap(v[2], v[6]);
    view_cswap(v[1], v[4]); view_cswap(v[3], v[6]);
    view_cswap(v[2], v[4]); view_cswap(v[3], v[5]);
    view_cswap(v[3], v[4]);
    const int lo = (K - 1) >> 1, hi = K >> 1;
    double a = v[0], b = v[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        if (i == lo) a = v[i];
        if (i == hi) b = v[i];
    }
    return (K & 1) ? a : 0.5 * (a + b);
}

// One wave per row r, lane j < J owning joint j: the own pose and at most VIEW_MAX_PEERS transformed peers in registers (every index a
// constant: the loops are unrolled and guarded by k <= np, which is uniform over the wave), the fused joint, then the squared distances
// of the contributions to it, added over the wave.  A row's 3 J floats are consecutive, so the wave's loads and stores are coalesced.
__global__ __launch_bounds__(256) void view_fuse_kernel(const float* __restrict__ pose, int F, int J, const int* __restrict__ peer_start,
                                                        const int* __restrict__ peer_row, const int* __restrict__ peer_fit,
                                                        const double* __restrict__ fit, int mode, float* __restrict__ fused,
                                                        float* __restrict__ disagreement) {
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (r >= F) return;
    const int p0 = peer_start[r];
    int np = peer_start[r + 1] - p0;
    np = np < 0 ? 0 : (np > VIEW_MAX_PEERS ? VIEW_MAX_PEERS : np);
    const bool on = lane < J;
    const int j = on ? lane : 0;                                                // idle lanes follow joint 0 and store nothing
    const size_t at = ((size_t)r * J + j) * 3;
    const float o0 = pose[at], o1 = pose[at + 1], o2 = pose[at + 2];
    if (np == 0) {
        if (on) {
            fused[at] = o0;
            fused[at + 1] = o1;
            fused[at + 2] = o2;
        }
        if (lane == 0) disagreement[r] = 0.0f;
        return;
    }
    const double inf = __builtin_huge_val();
    double c[VIEW_MAX_PEERS + 1][3];
    c[0][0] = (double)o0; c[0][1] = (double)o1; c[0][2] = (double)o2;
#pragma unroll
    for (int k = 1; k <= VIEW_MAX_PEERS; ++k) {
        c[k][0] = c[k][1] = c[k][2] = inf;
        if (k <= np) {
            const float* __restrict__ q = pose + ((size_t)peer_row[p0 + k - 1] * J + j) * 3;
            view_transform(fit + (size_t)peer_fit[p0 + k - 1] * VIEW_FIT_SLOTS, (double)q[0], (double)q[1], (double)q[2], c[k]);
        }
    }
    const int K = np + 1;
    double f[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        if (mode == 1) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = c[k][u];
            f[u] = view_median8(v, K);
        } else {
            double s = mode == 0 ? c[0][u] + c[1][u] : c[1][u];
#pragma unroll
            for (int k = 2; k <= VIEW_MAX_PEERS; ++k)
                if (k <= np) s += c[k][u];
            f[u] = s / (double)(mode == 0 ? K : np);
        }
    }
    double e = 0.0;
#pragma unroll
    for (int k = 0; k <= VIEW_MAX_PEERS; ++k) {
        if (k <= np) {
            const double d0 = c[k][0] - f[0], d1 = c[k][1] - f[1], d2 = c[k][2] - f[2];
            e += (d0 * d0 + d1 * d1) + d2 * d2;
        }
    }
    e = wave_sum_f64(on ? e : 0.0);
    if (on) {
        fused[at] = (float)f[0];
        fused[at + 1] = (float)f[1];
        fused[at + 2] = (float)f[2];
    }
    if (lane == 0) disagreement[r] = (float)sqrt(e / ((double)K * (double)J));
}
