// Temporal smoothing and constant bone lengths for stitched pose sequences (include/r50_smooth.h).
// Included after kernels.h (wave_sum_f64).  Everything is fp64 arithmetic on fp32 poses with one rounding at the store; the library is
// built with -ffp-contract=off, so every product and every sum below is rounded on its own.  No atomics anywhere.
#pragma once

#define SMOOTH_MAX_W 63
#define SMOOTH_MAX_J 64
#define FIR_ROWS 64                                                             // consecutive rows per workgroup of fir_sequences_kernel

// The sum of v over the 64 lanes of a wave in a fixed tree, valid in lane 0.
__device__ inline int wave_sum_i32(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// out[r] = sum_k coef[e][k] * x[lo + k] over the row's segment (see r50_smooth.h).  Workgroup b owns the rows [64 b, 64 b + 64) and walks
// their (row, component) elements in order, so a wave's loads at one tap are consecutive floats; the rows a neighbouring element read
// come back from the cache (an edge row's window reaches 2 R rows away, so a halo of R rows in LDS would not cover it; the table, read
// W times per element, is what sits in LDS).  Workgroup 0 also counts the rows of the segments shorter than W.
__global__ __launch_bounds__(256) void fir_sequences_kernel(const float* __restrict__ x, const int* __restrict__ seg_start,
                                                            const int* __restrict__ row_seg, int F, int G, int C,
                                                            const double* __restrict__ coef, int W, float* __restrict__ out,
                                                            int* __restrict__ short_rows) {
    __shared__ double cf[SMOOTH_MAX_W * SMOOTH_MAX_W];
    __shared__ int red[2][4];
    const int tid = threadIdx.x;
    for (int i = tid; i < W * W; i += 256) cf[i] = coef[i];
    __syncthreads();
    const int R = (W - 1) >> 1;
    const int r0 = blockIdx.x * FIR_ROWS;
    const int rows = F - r0 < FIR_ROWS ? F - r0 : FIR_ROWS;
    for (int i = tid; i < rows * C; i += 256) {
        const int r = r0 + i / C, c = i % C;
        const int g = row_seg[r];
        const int s0 = seg_start[g], L = seg_start[g + 1] - s0;
        const size_t at = (size_t)r * C + c;
        if (L < W) {
            out[at] = x[at];
            continue;
        }
        const int pos = r - s0;
        int lo = pos - R;
        lo = lo < 0 ? 0 : lo;
        lo = lo > L - W ? L - W : lo;
        const double* __restrict__ w = cf + (pos - lo) * W;
        const float* __restrict__ p = x + (size_t)(s0 + lo) * C + c;
        double acc = 0.0;
        for (int k = 0; k < W; ++k) acc += w[k] * (double)p[(size_t)k * C];
        out[at] = (float)acc;
    }
    if (blockIdx.x == 0) {
        int nr = 0, ns = 0;
        for (int g = tid; g < G; g += 256) {
            const int L = seg_start[g + 1] - seg_start[g];
            if (L < W) {
                nr += L;
                ns += 1;
            }
        }
        nr = wave_sum_i32(nr);
        ns = wave_sum_i32(ns);
        if ((tid & 63) == 0) {
            red[0][tid >> 6] = nr;
            red[1][tid >> 6] = ns;
        }
        __syncthreads();
        if (tid < 2) short_rows[tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
    }
}

#define EURO_AHEAD 4                                                            // rows loaded ahead of the recurrence

__device__ inline double one_euro_alpha(double fc, double te) { return 1.0 / (1.0 + 1.0 / ((6.283185307179586 * fc) * te)); }

// One wave per (segment, slab of 64 components): lane c walks x[s0 .. s1)[c0 + c].  A step is two dependent fp64 divisions long, so the
// kernel is bound by latency times the segment length, not by memory; the loads do not depend on the recurrence and are issued
// EURO_AHEAD rows early, so they hide behind it.
__global__ __launch_bounds__(256) void one_euro_sequences_kernel(const float* __restrict__ x, const int* __restrict__ seg_start, int G,
                                                                 int C, int slabs, double rate, double min_cutoff, double beta,
                                                                 double d_cutoff, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (wv >= G * slabs) return;
    const int g = wv / slabs, c = (wv - g * slabs) * 64 + lane;
    if (c >= C) return;
    const int s0 = seg_start[g], L = seg_start[g + 1] - s0;
    if (L < 1) return;
    const float* __restrict__ p = x + (size_t)s0 * C + c;
    float* __restrict__ q = out + (size_t)s0 * C + c;
    const double te = 1.0 / rate;
    const double ad = one_euro_alpha(d_cutoff, te);
    const float first = p[0];
    q[0] = first;
    double xhat = (double)first, dxhat = 0.0;
    float nxt[EURO_AHEAD];
#pragma unroll
    for (int u = 0; u < EURO_AHEAD; ++u) nxt[u] = 1 + u < L ? p[(size_t)(1 + u) * C] : 0.0f;
    for (int t = 1; t < L; t += EURO_AHEAD) {
        float cur[EURO_AHEAD];
#pragma unroll
        for (int u = 0; u < EURO_AHEAD; ++u) {
            cur[u] = nxt[u];
            nxt[u] = t + EURO_AHEAD + u < L ? p[(size_t)(t + EURO_AHEAD + u) * C] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < EURO_AHEAD; ++u) {
            if (t + u < L) {
                const double xt = (double)cur[u];
                const double dx = (xt - xhat) * rate;
                dxhat = dxhat + ad * (dx - dxhat);
                const double fc = min_cutoff + beta * fabs(dxhat);
                xhat = xhat + one_euro_alpha(fc, te) * (xt - xhat);
                q[(size_t)(t + u) * C] = (float)xhat;
            }
        }
    }
}

struct BoneEdges { unsigned char parent[SMOOTH_MAX_J], child[SMOOTH_MAX_J]; };   // by value in the kernel arguments (checked on the host)

__device__ inline double bone_length(const float* __restrict__ row, int pa, int ch) {
    const double dx = (double)row[3 * ch] - (double)row[3 * pa];
    const double dy = (double)row[3 * ch + 1] - (double)row[3 * pa + 1];
    const double dz = (double)row[3 * ch + 2] - (double)row[3 * pa + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// The sum of v over the 256 threads in a fixed tree (wave, then ((w0 + w1) + w2) + w3), returned to every thread.
__device__ inline double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    __syncthreads();                                                            // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup per sequence; per edge two passes over the sequence's rows (the mean, then the squared deviations from it), thread t
// taking the rows s0 + t, s0 + t + 256, ... in that order.
__global__ __launch_bounds__(256) void bone_stats_kernel(const float* __restrict__ x, const int* __restrict__ seq_start, int C, BoneEdges ed,
                                                         int E, double* __restrict__ stats) {
    __shared__ double red[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int s0 = seq_start[s], n = seq_start[s + 1] - s0;
    for (int b = 0; b < E; ++b) {
        const int pa = ed.parent[b], ch = ed.child[b];
        double a = 0.0;
        for (int r = tid; r < n; r += 256) a += bone_length(x + (size_t)(s0 + r) * C, pa, ch);
        const double mean = n > 0 ? block_sum_f64(a, red) / (double)n : 0.0;
        double d2 = 0.0;
        for (int r = tid; r < n; r += 256) {
            const double d = bone_length(x + (size_t)(s0 + r) * C, pa, ch) - mean;
            d2 += d * d;
        }
        const double ssd = n > 0 ? block_sum_f64(d2, red) : 0.0;
        if (tid == 0) {
            stats[((size_t)s * E + b) * 2] = mean;
            stats[((size_t)s * E + b) * 2 + 1] = ssd;
        }
    }
}

__host__ __device__ inline int bone_rebuild_rows(int J) { return J <= 28 ? 64 : 16; }                 // rows per workgroup: LDS <= 64 KB
__host__ __device__ inline int bone_rebuild_pitch(int C) { return C | 1; }                            // odd: lanes on distinct banks
__host__ __device__ inline size_t bone_rebuild_lds(int J) {
    return (size_t)bone_rebuild_rows(J) * ((size_t)3 * J * sizeof(double) + (size_t)bone_rebuild_pitch(3 * J) * sizeof(float));
}

// RB rows per workgroup of 64: the rows are staged in LDS as fp32 (xs, row-major with an odd pitch) by coalesced loads, lane l < RB then
// walks the edge list of row l with the rebuilt joints in fp64 (ps, component-major: ps[jc * RB + l]), and the workgroup stores the rows
// coalesced: a joint that is some edge's child from ps, rounded once, every other joint from xs, bit for bit.
__global__ __launch_bounds__(64) void bone_rebuild_kernel(const float* __restrict__ x, const int* __restrict__ row_seq, int F, int J,
                                                          BoneEdges ed, int E, unsigned long long is_child,
                                                          const double* __restrict__ stats, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bone_sm[];
    const int C = 3 * J, RB = bone_rebuild_rows(J), XP = bone_rebuild_pitch(C);
    double* ps = reinterpret_cast<double*>(bone_sm);
    float* xs = reinterpret_cast<float*>(bone_sm + (size_t)RB * C * sizeof(double));
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * RB;
    const int rows = F - r0 < RB ? F - r0 : RB;
    const float* __restrict__ src = x + (size_t)r0 * C;
    for (int i = tid; i < rows * C; i += 64) {
        const int l = i / C, jc = i - l * C;
        const float v = src[i];
        xs[l * XP + jc] = v;
        ps[jc * RB + l] = (double)v;
    }
    __syncthreads();
    if (tid < rows) {
        const double* __restrict__ len = stats + (size_t)row_seq[r0 + tid] * E * 2;
        const float* row = xs + tid * XP;
        for (int b = 0; b < E; ++b) {
            const int pa = ed.parent[b], ch = ed.child[b];
            const double dx = (double)row[3 * ch] - (double)row[3 * pa];
            const double dy = (double)row[3 * ch + 1] - (double)row[3 * pa + 1];
            const double dz = (double)row[3 * ch + 2] - (double)row[3 * pa + 2];
            const double nrm = sqrt((dx * dx + dy * dy) + dz * dz);
            const double lb = len[2 * b];
            const double px = ps[(3 * pa) * RB + tid], py = ps[(3 * pa + 1) * RB + tid], pz = ps[(3 * pa + 2) * RB + tid];
            const bool zero = nrm == 0.0;
            ps[(3 * ch) * RB + tid] = px + (zero ? dx : (lb * dx) / nrm);
            ps[(3 * ch + 1) * RB + tid] = py + (zero ? dy : (lb * dy) / nrm);
            ps[(3 * ch + 2) * RB + tid] = pz + (zero ? dz : (lb * dz) / nrm);
        }
    }
    __syncthreads();
    float* __restrict__ dst = out + (size_t)r0 * C;
    for (int i = tid; i < rows * C; i += 64) {
        const int l = i / C, jc = i - l * C;
        dst[i] = ((is_child >> (jc / 3)) & 1ull) ? (float)ps[jc * RB + l] : xs[l * XP + jc];
    }
}
