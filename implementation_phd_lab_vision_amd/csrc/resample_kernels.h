// A pose at any time stamp from the rows around it (include/r50_resample.h, INTEGRATION.md section AB).
// Everything is fp64 arithmetic on fp32 poses with one rounding at the store; the library is built with -ffp-contract=off, so every
// product, quotient and sum below is rounded on its own, in the order r50_resample.h writes it.  No atomics anywhere.
#pragma once

#define RESAMPLE_MAX_J 64
#define RESAMPLE_BLOCK 256                                                      // output elements (and threads) per workgroup
#define RESAMPLE_MAX_ROWS (RESAMPLE_BLOCK / 3 + 2)                              // rows a workgroup's 256 elements can lie in (C >= 3)

#define RESAMPLE_COPY 0                                                         // how a row is made: one source row's bits,
#define RESAMPLE_LERP 1                                                         // the linear form,
#define RESAMPLE_HERMITE 2                                                      // or the cubic one
#define RESAMPLE_HAS_LEFT 1                                                     // [i-1, i] is inside the sequence and bridged
#define RESAMPLE_HAS_RIGHT 2                                                    // [i+1, i+2] likewise

// What one output row needs beyond its source values, formed once per row.  w[]: u for the linear form; h00, h10 * h, h01, h11 * h
// for the cubic one.  h, hl, hr: idx[i+1] - idx[i], idx[i] - idx[i-1], idx[i+2] - idx[i+1] (the latter two where the bits of
// `sides` say so).
struct ResampleRow {
    double w[4];
    double h, hl, hr;
    int row;                                                                    // i, or the row to copy
    int how, sides;
    int pad;
};

__device__ inline ResampleRow resample_row(const int* __restrict__ idx, const int* __restrict__ seq_start, double tau, int s, int i,
                                           int kind, int max_gap, int& flag) {
    ResampleRow r;
    r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0.0;
    r.h = r.hl = r.hr = 1.0;
    r.row = i;
    r.how = RESAMPLE_COPY;
    r.sides = 0;
    r.pad = 0;
    flag = 0;
    const int a = seq_start[s], b = seq_start[s + 1];
    const long long ti = idx[i];
    const double t0 = (double)ti;
    if (tau == t0) return r;
    if (tau < t0 || i + 1 >= b) {                                               // before the first stamp (i == a) or after the last
        flag = 2;
        return r;
    }
    const long long gap = (long long)idx[i + 1] - ti;
    if (gap > (long long)max_gap) {                                             // inside a break: the nearer knot, the left one on a tie
        flag = 1;
        if (!((tau - t0) <= ((double)idx[i + 1] - tau))) r.row = i + 1;
        return r;
    }
    const double h = (double)gap;
    const double u = (tau - t0) / h;
    r.h = h;
    if (kind == 0) {
        r.how = RESAMPLE_LERP;
        r.w[0] = u;
        return r;
    }
    r.how = RESAMPLE_HERMITE;
    const double u2 = u * u;
    const double u3 = u2 * u;
    r.w[0] = ((2.0 * u3) - (3.0 * u2)) + 1.0;
    r.w[1] = ((u3 - (2.0 * u2)) + u) * h;
    r.w[2] = (-(2.0 * u3)) + (3.0 * u2);
    r.w[3] = (u3 - u2) * h;
    if (i - 1 >= a) {
        const long long gl = ti - (long long)idx[i - 1];
        if (gl <= (long long)max_gap) {
            r.sides |= RESAMPLE_HAS_LEFT;
            r.hl = (double)gl;
        }
    }
    if (i + 2 < b) {
        const long long gr = (long long)idx[i + 2] - (long long)idx[i + 1];
        if (gr <= (long long)max_gap) {
            r.sides |= RESAMPLE_HAS_RIGHT;
            r.hr = (double)gr;
        }
    }
    return r;
}

// Workgroup k owns the elements [256 k, 256 k + 256) of y (G, C).  Phase 1: thread t < (rows these lie in) forms the record of row
// r0 + t in LDS and stores its flag (a row's flag is stored by the workgroup its FIRST element lies in, so once).  Phase 2: thread t
// makes element 256 k + t from its row's record and x[row-1 .. row+2][c]; the source rows of neighbouring output rows overlap and
// come back from the cache.
__global__ __launch_bounds__(RESAMPLE_BLOCK) void resample_sequences_kernel(const float* __restrict__ x, const int* __restrict__ idx,
                                                                            const int* __restrict__ seq_start, int C,
                                                                            const double* __restrict__ out_time,
                                                                            const int* __restrict__ out_seq,
                                                                            const int* __restrict__ out_left, int G, int kind, int max_gap,
                                                                            float* __restrict__ y, int* __restrict__ flags) {
    __shared__ ResampleRow rows[RESAMPLE_MAX_ROWS];
    const int tid = threadIdx.x;
    const int total = G * C;                                                    // < 2^31: G < 2^31 / 192
    const int e0 = blockIdx.x * RESAMPLE_BLOCK;
    const int e1 = e0 + RESAMPLE_BLOCK < total ? e0 + RESAMPLE_BLOCK : total;   // e0 < total by the grid
    const int r0 = e0 / C, r1 = (e1 - 1) / C;
    if (tid <= r1 - r0) {
        const int g = r0 + tid;
        int flag;
        rows[tid] = resample_row(idx, seq_start, out_time[g], out_seq[g], out_left[g], kind, max_gap, flag);
        if (g * C >= e0) flags[g] = flag;
    }
    __syncthreads();
    const int e = e0 + tid;
    if (e >= total) return;
    const int g = e / C, c = e - g * C;
    const ResampleRow& r = rows[g - r0];
    const float* __restrict__ p = x + (size_t)r.row * C + c;
    if (r.how == RESAMPLE_COPY) {
        y[e] = p[0];
        return;
    }
    const double x0 = (double)p[0], x1 = (double)p[C];
    if (r.how == RESAMPLE_LERP) {
        y[e] = (float)((x0 + r.w[0] * (x1 - x0)) + 0.0);
        return;
    }
    const double d01 = (x1 - x0) / r.h;
    const bool left = r.sides & RESAMPLE_HAS_LEFT, right = r.sides & RESAMPLE_HAS_RIGHT;
    double dm = 0.0, dp = 0.0;
    if (left) dm = (x0 - (double)p[-C]) / r.hl;
    if (right) dp = ((double)p[2 * C] - x1) / r.hr;
    double m0, m1;
    if (left) m0 = (r.h * dm + r.hl * d01) / (r.hl + r.h);
    else if (right) m0 = (((2.0 * r.h) + r.hr) * d01 - r.h * dp) / (r.h + r.hr);
    else m0 = d01;
    if (right) m1 = (r.hr * d01 + r.h * dp) / (r.h + r.hr);
    else if (left) m1 = (((2.0 * r.h) + r.hl) * d01 - r.h * dm) / (r.h + r.hl);
    else m1 = d01;
    y[e] = (float)((((r.w[0] * x0 + r.w[1] * m0) + r.w[2] * x1) + r.w[3] * m1) + 0.0);
}
