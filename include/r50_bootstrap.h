/*
 * r50_bootstrap.h — C ABI of libr50hip.so, ninth public header: the stratified cluster bootstrap of per-unit metric sums, for
 * confidence intervals on the numbers `results` prints and for the paired comparison of two models (INTEGRATION.md section AC).
 *
 * A cache cuts a video into overlapping clips, so the clips of a take are strongly dependent and a standard error over clips
 * overstates the certainty.  The bootstrap here resamples whole units (sequences, takes or clips) with replacement inside each
 * stratum (an action) and recomputes the sums; with the columns of two models side by side the same units are drawn for both, so an
 * interval on the difference is paired.  The reference prints point values only, so the stage is this project's definition.  The
 * conventions are those of r50.h: plain pointers and sizes, 0 on success or a negative r50_status, the text of a refusal through
 * r50_last_error(NULL), every device pointer owned by the caller, the launch on `stream`.
 *
 * Operands
 *   v (U, M) fp64: one row per resampling unit, sorted by stratum; each column is a per-unit sum (an error sum, or a pose / clip count).
 *   stratum_start (G+1) int32, device memory and trusted as seq_start is in r50_smooth.h: the caller checks it on the host
 *   (bootstrap.UnitTable does) and uploads it.  Stratum g is the rows a_g = stratum_start[g] .. b_g - 1 = stratum_start[g+1] - 1,
 *   n_g = b_g - a_g >= 1, stratum_start[0] = 0, stratum_start[G] = U.
 *
 * Draws (stratified)
 *   Replicate rho = r0 + r (r in [0, R)) takes n_g draws from stratum g.  Draw k of stratum g has the global position i = a_g + k.
 *   Its 32-bit word is word (i & 3) of Philox4x32-10 (Salmon et al., SC 2011; multipliers D2511F53 / CD9E8D57, key increments
 *   9E3779B9 / BB67AE85) with
 *     key     (lo32(seed), hi32(seed))
 *     counter (lo32(i >> 2), 0, lo32(rho), hi32(rho)).
 *   The unit it names is a_g + (((uint64_t)word * n_g) >> 32): multiply-shift, no rejection.  A unit is named by floor or ceil of
 *   2^32 / n_g of the 2^32 words, so its probability deviates from 1 / n_g by at most 2^-32 in absolute terms (relative to 1 / n_g
 *   that is n_g * 2^-32 <= 2^-8 at the largest stratum the op admits, and 1.7e-6 at a stratum of 7,000 clips).
 *   c[rho][u] is the number of draws of replicate rho that name unit u; the c of a stratum sum to n_g.
 *   Replicate rho is a pure function of (seed, rho): launches over [r0, r0 + R) may be cut anywhere (chunks, several devices) and give
 *   the same bits.
 *
 * Output
 *   out[r, g, m] = sum over u = a_g .. b_g - 1, ascending, of (double)c[u] * v[u, m]; the sum starts at +0.0, units with c[u] = 0 are
 *   skipped, every product and every add is rounded on its own (the library is built with -ffp-contract=off).
 */
#ifndef R50_BOOTSTRAP_H_
#define R50_BOOTSTRAP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R50_BOOTSTRAP_MAX_UNITS (1 << 24)
#define R50_BOOTSTRAP_MAX_COLUMNS 4096
#define R50_BOOTSTRAP_MAX_WINDOW 32768

/* out (R, G, M) fp64, every element written; counts, if not NULL, (R, U) int32 receives c, every element written.
 *    One workgroup of 256 per (replicate, stratum): grid (G, min(R, 65535), ceil(R / 65535)), a function of R and G alone, not
 *    persistent.  The multiplicities of the stratum are built in LDS as 32-bit integers with integer LDS atomics (integer adds commute:
 *    the same bits whatever their order); dynamic LDS is 4 * min(window, U) bytes.  A stratum of more than `window` units is done in
 *    passes over windows of `window` units: each pass regenerates the stratum's draws and continues the same ascending sum, so the bits
 *    do not depend on `window`.  One Philox block serves four consecutive draws.  The sums run one column per lane, loads of v coalesced
 *    along M; M above 256 loops over column chunks (each regenerates the draws).  No floating-point atomic, no global atomic, no
 *    scratch, no host read, no allocation: the same bits on every run.
 *    Refused before any launch: a NULL v, stratum_start or out; U, G, M or R < 1; G > U; U > 2^24; M > 4096; r0 < 0 or r0 + R
 *    overflowing int64; R * G * M or R * U >= 2^40 (and R > 65535^2, the grid's reach); window outside [1, 32768]; v or out not 8-byte aligned (counts not 4-byte
 *    aligned); out or counts overlapping an input or each other. */
int r50_op_bootstrap_sums(const double* v, const int* stratum_start, int64_t U, int G, int M, int64_t r0, int64_t R, uint64_t seed,
                          int window, double* out, int* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R50_BOOTSTRAP_H_ */
