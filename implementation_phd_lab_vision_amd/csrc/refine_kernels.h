// 2D-guided refinement of stitched pose sequences (include/r50_refine.h).
// Included after smooth_kernels.h (BoneEdges, block_sum_f64, SMOOTH_MAX_J).  Everything is fp64 arithmetic with one rounding at the final
// store; the library is built with -ffp-contract=off, so every product and every sum below is rounded on its own.  No atomics anywhere.
#pragma once

#define FIT_MAX_J SMOOTH_MAX_J
#define FIT_HALO 2                                                              // rows staged in front of and behind a workgroup's own

__host__ __device__ inline int pose_fit_rows(int J) { return J <= 32 ? 64 : 32; }                     // rows per workgroup: LDS <= 64 KB
__host__ __device__ inline size_t pose_fit_lds(int J) {
    const int rb = pose_fit_rows(J);
    return (size_t)(rb + 2 * FIT_HALO) * 3 * J * sizeof(double) + (size_t)3 * rb * sizeof(int);
}

// Per joint, the edges it is an endpoint of in edge-list order: entries adj_start[j] .. adj_start[j+1]-1 of (edge, other endpoint).
// Built on the host from the checked edge list; by value in the kernel arguments.
struct FitAdjacency {
    unsigned char start[FIT_MAX_J + 1];
    unsigned char edge[2 * (FIT_MAX_J - 1)];
    unsigned char other[2 * (FIT_MAX_J - 1)];
};

struct FitParams { double l2d, l3d, lacc, lbone, omega, z_min; };

// One damped block-Jacobi Gauss-Newton sweep (see r50_refine.h for the definition and the order of every sum).  Workgroup b owns the rows
// [RB b, RB b + RB) and stages them with FIT_HALO rows on either side in LDS as fp64 (from the fp32 x0 in the first sweep, from the previous
// iterate after it), so a stencil and a bone read neighbours from LDS only; the (row, joint) elements of the block are then walked in
// order by the 256 threads, each element by one thread, so loads and stores of consecutive lanes are consecutive.  A stencil is used only
// if its three rows lie in the row's segment, so a staged row of another segment (or the zero rows outside [0, F)) is never read.
template <bool SRC32, bool DST32>
__global__ __launch_bounds__(256) void pose_fit_sweep_kernel(const float* __restrict__ x0, const double* __restrict__ src,
                                                             const float* __restrict__ rays, const float* __restrict__ conf,
                                                             const int* __restrict__ seg_start, const int* __restrict__ row_seg,
                                                             const int* __restrict__ row_seq, int F, int J, FitAdjacency adj, int E,
                                                             const double* __restrict__ bone_len, FitParams pr,
                                                             double* __restrict__ dst, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fit_sm[];
    const int C = 3 * J, RB = pose_fit_rows(J);
    double* tile = reinterpret_cast<double*>(fit_sm);                           // (RB + 4) rows of C doubles; row r0 - 2 first
    int* lo = reinterpret_cast<int*>(fit_sm + (size_t)(RB + 2 * FIT_HALO) * C * sizeof(double));
    int* hi = lo + RB;
    int* sq = hi + RB;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * RB;
    const int rows = F - r0 < RB ? F - r0 : RB;
    const int first = r0 - FIT_HALO < 0 ? 0 : r0 - FIT_HALO;
    const int last = r0 + rows + FIT_HALO > F ? F : r0 + rows + FIT_HALO;       // one past the last staged row
    {
        const size_t base = (size_t)first * C;
        double* t0 = tile + (size_t)(first - (r0 - FIT_HALO)) * C;
        const int n = (last - first) * C;
        for (int i = tid; i < n; i += 256) t0[i] = SRC32 ? (double)x0[base + i] : src[base + i];
    }
    for (int l = tid; l < rows; l += 256) {
        const int g = row_seg[r0 + l];
        lo[l] = seg_start[g];
        hi[l] = seg_start[g + 1];
        sq[l] = pr.lbone != 0.0 ? row_seq[r0 + l] : 0;
    }
    __syncthreads();
    for (int i = tid; i < rows * J; i += 256) {
        const int l = i / J, j = i - l * J;
        const int t = r0 + l;
        const size_t at = (size_t)t * J + j;
        const double* __restrict__ row = tile + (size_t)(l + FIT_HALO) * C;
        const double px = row[3 * j], py = row[3 * j + 1], pz = row[3 * j + 2];
        const double p0x = (double)x0[3 * at], p0y = (double)x0[3 * at + 1], p0z = (double)x0[3 * at + 2];
        double gx = 0.0, gy = 0.0, gz = 0.0;
        double h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0;
        // term 1: the reprojection residual in metres at the depth of the prediction
        const double w = pr.l2d != 0.0 ? pr.l2d * (conf ? (double)conf[at] : 1.0) : 0.0;
        if (w != 0.0 && pz >= pr.z_min) {
            const double z0 = p0z > pr.z_min ? p0z : pr.z_min;
            const double s = z0 / pz, qx = px / pz, qy = py / pz;
            const double rx = z0 * (qx - (double)rays[2 * at]), ry = z0 * (qy - (double)rays[2 * at + 1]);
            const double ss = s * s;
            gx = w * (s * rx);
            gy = w * (s * ry);
            gz = w * (s * (-(qx * rx + qy * ry)));
            h00 = w * ss;
            h02 = w * (ss * (-qx));
            h11 = w * ss;
            h12 = w * (ss * (-qy));
            h22 = w * (ss * (qx * qx + qy * qy));
        }
        // term 2: the distance to the prediction
        gx += pr.l3d * (px - p0x);
        gy += pr.l3d * (py - p0y);
        gz += pr.l3d * (pz - p0z);
        double hd = pr.l3d;
        // term 3: the second differences centred at t - 1, t, t + 1 that lie in the segment
        if (pr.lacc != 0.0) {
            const int s0 = lo[l], s1 = hi[l];
            double ax = 0.0, ay = 0.0, az = 0.0, kk = 0.0;
#pragma unroll
            for (int d = -1; d <= 1; ++d) {
                const int c = t + d;
                if (c - 1 < s0 || c + 1 >= s1) continue;
                const double k = d == 0 ? -2.0 : 1.0;
                const double* __restrict__ a = row + (d - 1) * C + 3 * j;
                const double* __restrict__ b = row + d * C + 3 * j;
                const double* __restrict__ e = row + (d + 1) * C + 3 * j;
                ax += k * ((a[0] - 2.0 * b[0]) + e[0]);
                ay += k * ((a[1] - 2.0 * b[1]) + e[1]);
                az += k * ((a[2] - 2.0 * b[2]) + e[2]);
                kk += k * k;
            }
            gx += pr.lacc * ax;
            gy += pr.lacc * ay;
            gz += pr.lacc * az;
            hd += pr.lacc * kk;
        }
        h00 += hd;
        h11 += hd;
        h22 += hd;
        // term 4: the bones that end at this joint, in edge-list order
        if (pr.lbone != 0.0) {
            const double* __restrict__ len = bone_len + (size_t)sq[l] * E;
            double bx = 0.0, by = 0.0, bz = 0.0, u00 = 0.0, u01 = 0.0, u02 = 0.0, u11 = 0.0, u12 = 0.0, u22 = 0.0;
            for (int q = adj.start[j]; q < adj.start[j + 1]; ++q) {
                const int o = adj.other[q];
                const double dx = px - row[3 * o], dy = py - row[3 * o + 1], dz = pz - row[3 * o + 2];
                const double L = sqrt((dx * dx + dy * dy) + dz * dz);
                if (L == 0.0) continue;
                const double ux = dx / L, uy = dy / L, uz = dz / L;
                const double m = L - len[adj.edge[q]];
                bx += m * ux;
                by += m * uy;
                bz += m * uz;
                u00 += ux * ux;
                u01 += ux * uy;
                u02 += ux * uz;
                u11 += uy * uy;
                u12 += uy * uz;
                u22 += uz * uz;
            }
            gx += pr.lbone * bx;
            gy += pr.lbone * by;
            gz += pr.lbone * bz;
            h00 += pr.lbone * u00;
            h01 += pr.lbone * u01;
            h02 += pr.lbone * u02;
            h11 += pr.lbone * u11;
            h12 += pr.lbone * u12;
            h22 += pr.lbone * u22;
        }
        // H = L D L^T without pivoting (H is positive definite: lambda_3d > 0), then the two triangular solves
        const double l10 = h01 / h00, l20 = h02 / h00;
        const double d1 = h11 - l10 * h01;
        const double m12 = h12 - l20 * h01;
        const double l21 = m12 / d1;
        const double d2 = h22 - (l20 * h02 + l21 * m12);
        const double y1 = gy - l10 * gx;
        const double y2 = gz - (l20 * gx + l21 * y1);
        const double sz = y2 / d2;
        const double sy = y1 / d1 - l21 * sz;
        const double sx = gx / h00 - (l10 * sy + l20 * sz);
        const double nx = px - pr.omega * sx, ny = py - pr.omega * sy, nz = pz - pr.omega * sz;
        if (DST32) {
            out[3 * at] = (float)nx;
            out[3 * at + 1] = (float)ny;
            out[3 * at + 2] = (float)nz;
        } else {
            dst[3 * at] = nx;
            dst[3 * at + 1] = ny;
            dst[3 * at + 2] = nz;
        }
    }
}

// The launch of one sweep: the grid is a function of F and J alone.
template <bool SRC32, bool DST32>
inline void launch_fit_sweep(const float* x0, const double* src, const float* rays, const float* conf, const int* seg_start, const int* row_seg,
                             const int* row_seq, int F, int J, const FitAdjacency& adj, int E, const double* bone_len, const FitParams& pr,
                             double* dst, float* out, hipStream_t stream) {
    const int rb = pose_fit_rows(J);
    hipLaunchKernelGGL((pose_fit_sweep_kernel<SRC32, DST32>), dim3((unsigned)((F + rb - 1) / rb)), dim3(256), pose_fit_lds(J), stream, x0, src,
                       rays, conf, seg_start, row_seg, row_seq, F, J, adj, E, bone_len, pr, dst, out);
}

#define FIT_ENERGY_SLOTS 6

// One workgroup of 256 per sequence: thread t scores the rows s0 + t, s0 + t + 256, ... in that order (per row the joints ascending, then
// the edges in list order), one running sum per slot, then a fixed tree over the wave and the four waves.
__global__ __launch_bounds__(256) void pose_fit_energy_kernel(const float* __restrict__ x, const float* __restrict__ x0,
                                                              const float* __restrict__ rays, const float* __restrict__ conf,
                                                              const int* __restrict__ seq_start, const int* __restrict__ row_seg, int J,
                                                              BoneEdges ed, int E, const double* __restrict__ bone_len, double z_min,
                                                              double* __restrict__ energy) {
    __shared__ double red[4];
    const int s = blockIdx.x, tid = threadIdx.x, C = 3 * J;
    const int s0 = seq_start[s], s1 = seq_start[s + 1];
    double acc[FIT_ENERGY_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = s0 + tid; r < s1; r += 256) {
        const float* __restrict__ xr = x + (size_t)r * C;
        const float* __restrict__ pr = x0 + (size_t)r * C;
        const int g = row_seg[r];
        const bool mid = r - 1 >= s0 && r + 1 < s1 && row_seg[r - 1] == g && row_seg[r + 1] == g;
        for (int j = 0; j < J; ++j) {
            const double px = (double)xr[3 * j], py = (double)xr[3 * j + 1], pz = (double)xr[3 * j + 2];
            const double p0x = (double)pr[3 * j], p0y = (double)pr[3 * j + 1], p0z = (double)pr[3 * j + 2];
            if (pz >= z_min) {
                const double z0 = p0z > z_min ? p0z : z_min;
                const double cf = conf ? (double)conf[(size_t)r * J + j] : 1.0;
                const double rx = z0 * (px / pz - (double)rays[2 * ((size_t)r * J + j)]);
                const double ry = z0 * (py / pz - (double)rays[2 * ((size_t)r * J + j) + 1]);
                acc[0] += cf * (rx * rx + ry * ry);
                acc[4] += cf;
            } else {
                acc[5] += 1.0;
            }
            const double dx = px - p0x, dy = py - p0y, dz = pz - p0z;
            acc[1] += (dx * dx + dy * dy) + dz * dz;
            if (mid) {
                const double ax = ((double)xr[3 * j - C] - 2.0 * px) + (double)xr[3 * j + C];
                const double ay = ((double)xr[3 * j + 1 - C] - 2.0 * py) + (double)xr[3 * j + 1 + C];
                const double az = ((double)xr[3 * j + 2 - C] - 2.0 * pz) + (double)xr[3 * j + 2 + C];
                acc[2] += (ax * ax + ay * ay) + az * az;
            }
        }
        if (bone_len) {
            const double* __restrict__ len = bone_len + (size_t)s * E;
            for (int b = 0; b < E; ++b) {
                const double L = bone_length(xr, ed.parent[b], ed.child[b]);
                if (L == 0.0) continue;
                const double m = L - len[b];
                acc[3] += m * m;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < FIT_ENERGY_SLOTS; ++q) {
        const double v = block_sum_f64(acc[q], red);
        if (tid == 0) energy[(size_t)s * FIT_ENERGY_SLOTS + q] = v;
    }
}
