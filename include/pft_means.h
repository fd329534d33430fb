/*
 * pft_means.h -- f6: exact sums of u and p over the interior cells of a state (u, p, gl): the mean
 * temperature, the mean ice temperature next to pft_diag's ice_u_maxabs, the diffuse ice
 * saturation mean(p) over the pore space next to the thresholded ice / pore, and per interior
 * plane the horizontally averaged profiles <u>(z), <p>(z) -- what NCO's default ncwa (an average)
 * gives from a snapshot, without the download and without a summation order.
 *
 * Every sum is accumulated exactly, in integers (pft_xsum), so the record is the same bits for
 * every grid, thread count, arrival order and Z-decomposition, and one rounding at the end
 * (pft_xsum_round, or Python's integer division for a mean) gives the correctly rounded result.
 *
 * Conventions as pft_diag.h: extern "C"; every call returns int (0 = OK, -2 = bad arguments).
 * The device twin of pft_means_host is pft_slab_means (pft_hip.h), the solver-level collective
 * pft_solver_means (pft_solver.h).
 */
#ifndef PFT_MEANS_H
#define PFT_MEANS_H

#include "pft_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A fixed-point accumulator as wide as the doubles: value = sum_j w[j] * 2^(32 j - 1074), exactly.
   Adding one finite double x (E its biased exponent, M its 52 fraction bits plus the hidden bit
   when E != 0): b = max(E, 1) - 1, c = b >> 5, s = b & 31, T = M << s (at most 84 bits);
       w[c]     += +-(T & 0xffffffff)
       w[c + 1] += +-((T >> 32) & 0xffffffff)
       w[c + 2] += +-(T >> 64)
   with the sign of x; +-0 adds nothing.  The words are NOT carry-normalised: each is a plain sum
   of integers below 2^32 in magnitude, so the words of two accumulations of the same values are
   equal whatever the order, and a signed 64-bit word holds 2^31 contributions -- the records below
   are defined for at most 2^31 - 1 cells. */
#define PFT_XSUM_WORDS 66
typedef struct { long long w[PFT_XSUM_WORDS]; } pft_xsum;

/* the rule above; -2: NULL, or x is a NaN or +-Inf (nothing is added) */
int pft_xsum_add(pft_xsum * acc, double x);
/* into += other, word by word; -2: NULL */
int pft_xsum_combine(pft_xsum * into, const pft_xsum * other);
/* *out = the exact sum rounded once, to nearest, ties to even: subnormal results are exact or
   correctly rounded, a sum past DBL_MAX's rounding range gives +-Inf, an exact zero +0.0.  Any
   words are accepted (carries are propagated in 128 bits).  -2: NULL */
int pft_xsum_round(const pft_xsum * acc, double * out);

enum { PFT_MEAN_U, PFT_MEAN_P, PFT_MEAN_U_ICE, PFT_MEAN_P_PORE, PFT_MEAN_COUNT };

typedef struct {
	long long n[PFT_MEAN_COUNT];      /* cells that entered each sum */
	pft_xsum sum[PFT_MEAN_COUNT];     /* U: u over all interior cells; P: p over all of them;
	                                     U_ICE: u over cells with p > p_thr; P_PORE: p over cells
	                                     with gl < gl_thr (strict, ordered comparisons as in pft_diag:
	                                     a NaN in p or gl is neither ice nor pore).  A cell whose
	                                     summand is a NaN or +-Inf is left out of that sum and of
	                                     its n; a zero of either sign is counted and adds nothing */
} pft_means;

/* The record of the interior of a host array in the reference's padded layout (pft_model.h); no
   ghost cell is read.  opts = NULL: thresholds 0.5.  per_plane (optional, g->n3 records): the
   record of each interior plane of this slab, entry k for the global row g->first_row + k; total
   is their word-wise sum.  OpenMP over the planes; integer sums, so the result does not depend on
   the thread count.  0, or -2 (NULL, a grid without cells or with more than 2^31 - 1). */
int pft_means_host(const pft_grid * g, const double * x_host_padded, const pft_diag_opts * opts,
                   pft_means * total, pft_means * per_plane);

/* into += other: counts and words add.  Associative and commutative bit for bit; a zeroed record
   is the neutral element.  0, or -2 (NULL). */
int pft_means_combine(pft_means * into, const pft_means * other);

#ifdef __cplusplus
}
#endif
#endif
