// Stratified cluster bootstrap of per-unit sums (include/r50_bootstrap.h, INTEGRATION.md section AC).
// The draws are Philox4x32-10 words, a pure function of (seed, replicate, position); the multiplicities of one (replicate, stratum) are
// a histogram of 32-bit integers in LDS (integer LDS atomics: integer adds commute, so the bits do not depend on their order); the sums
// are fp64, one column per lane, the units of a stratum in ascending order.  The library is built with -ffp-contract=off, so every
// product and every add below is rounded on its own.  No floating-point atomic, no global atomic, no scratch.
#pragma once

#include <stdint.h>

#define BOOT_BLOCK 256                                                          // threads per workgroup = columns per column chunk
#define BOOT_MAX_WINDOW 32768                                                   // units of a stratum whose multiplicities LDS holds at once
#define BOOT_MAX_M 4096
#define BOOT_GRID_Y 65535                                                       // replicate r = blockIdx.z * BOOT_GRID_Y + blockIdx.y

#define BOOT_PHILOX_M0 0xD2511F53u
#define BOOT_PHILOX_M1 0xCD9E8D57u
#define BOOT_PHILOX_W0 0x9E3779B9u
#define BOOT_PHILOX_W1 0xBB67AE85u

// Philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011).
__device__ inline void boot_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(BOOT_PHILOX_M0, c0), lo0 = BOOT_PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(BOOT_PHILOX_M1, c2), lo1 = BOOT_PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += BOOT_PHILOX_W0;
        k1 += BOOT_PHILOX_W1;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// Workgroup (blockIdx.x = g, blockIdx.y + 65535 blockIdx.z = r) makes out[r, g, :] and, with counts, counts[r, a_g .. b_g).
// Per column chunk of 256 columns (one for M <= 256) and per window of `window` units of the stratum:
//   1. hist[0 .. wn) = 0;
//   2. thread t takes the Philox blocks q = (a >> 2) + t, + 256, ... up to (b - 1) >> 2: one block serves the four positions 4 q .. 4 q + 3,
//      those inside [a, b) name a unit each, those whose unit lies in the window add 1 to its hist entry (ds_add_u32);
//   3. the first chunk stores hist to counts, coalesced;
//   4. thread t continues the sum of column m0 + t over the window's units in ascending order, eight loads of v in flight; hist[k] is one
//      address for the whole wave (a broadcast read), v[u, m0 .. m0 + 255] is coalesced along the columns.
// A later window or chunk regenerates the stratum's draws: the counter form needs no memory for that.
__global__ __launch_bounds__(BOOT_BLOCK) void bootstrap_sums_kernel(const double* __restrict__ v, const int* __restrict__ stratum_start,
                                                                    long long U, int G, int M, long long r0, long long R, uint32_t key0,
                                                                    uint32_t key1, int window, double* __restrict__ out,
                                                                    int* __restrict__ counts) {
    extern __shared__ int boot_hist[];
    const int tid = threadIdx.x;
    const int g = blockIdx.x;
    const long long r = (long long)blockIdx.z * BOOT_GRID_Y + blockIdx.y;
    if (r >= R) return;                                                         // the whole workgroup: before any barrier
    const unsigned long long rho = (unsigned long long)(r0 + r);
    const uint32_t rho_lo = (uint32_t)rho, rho_hi = (uint32_t)(rho >> 32);
    const int a = stratum_start[g], b = stratum_start[g + 1];
    const uint32_t n = (uint32_t)(b - a);
    const uint32_t q0 = (uint32_t)a >> 2, q1 = (uint32_t)(b - 1) >> 2;
    for (int m0 = 0; m0 < M; m0 += BOOT_BLOCK) {
        const int m = m0 + tid;
        const bool has_col = m < M;
        const double* __restrict__ col = v + (has_col ? m : 0);
        double acc = 0.0;
        for (uint32_t w0 = 0; w0 < n; w0 += (uint32_t)window) {
            const uint32_t wn = n - w0 < (uint32_t)window ? n - w0 : (uint32_t)window;
            for (uint32_t k = tid; k < wn; k += BOOT_BLOCK) boot_hist[k] = 0;
            __syncthreads();
            for (uint32_t q = q0 + tid; q <= q1; q += BOOT_BLOCK) {
                uint32_t w[4];
                boot_philox4x32_10(q, 0u, rho_lo, rho_hi, key0, key1, w);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t i = 4u * q + (uint32_t)j;
                    const uint32_t unit = __umulhi(w[j], n) - w0;               // in [0, n) before the shift; wraps high below the window
                    if (i >= (uint32_t)a && i < (uint32_t)b && unit < wn) atomicAdd(&boot_hist[unit], 1);
                }
            }
            __syncthreads();
            const long long u0 = (long long)a + w0;
            if (counts && m0 == 0)
                for (uint32_t k = tid; k < wn; k += BOOT_BLOCK) counts[r * U + u0 + k] = boot_hist[k];
            if (has_col) {
                const double* __restrict__ p = col + u0 * M;
                uint32_t k = 0;
                for (; k + 8 <= wn; k += 8) {
                    int c[8];
                    double x[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        c[j] = boot_hist[k + j];
                        x[j] = p[(long long)(k + j) * M];
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (c[j]) acc = acc + (double)c[j] * x[j];
                }
                for (; k < wn; ++k) {
                    const int c = boot_hist[k];
                    if (c) acc = acc + (double)c * p[(long long)k * M];
                }
            }
            __syncthreads();                                                    // the next window's zeroing follows the last read
        }
        if (has_col) out[(r * G + g) * M + m] = acc;
    }
}
