/*
 * pft_means.c -- f6: the exact accumulator and the means record on a host array
 * (include/pft_means.h): the host-layout twin of the device reduction (means_kernel,
 * pft_reduce.hip), which must give the same raw words.
 *
 * Host C99 (with the compiler's 128-bit integer), OpenMP over the planes like pft_diag_host.
 * Every word is a sum of integers, so the threads' records merge to the same bits in any order.
 */
#include "../../include/pft_means.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

typedef __int128 i128;

/* the three digits of |x| and their first word; 0 when x adds nothing (+-0), -1 when x is not
   finite */
static int xsum_digits(double x, int * c, uint64_t d[3], int * neg)
{
	uint64_t bits, M, lo, hi;
	int E, b, s;
	memcpy(&bits, &x, 8);
	E = (int)((bits >> 52) & 0x7ff);
	if(E == 0x7ff) return -1;
	M = bits & 0xfffffffffffffULL;
	if(E) M |= 1ULL << 52;
	if(!M) return 0;
	b = (E > 1 ? E : 1) - 1;
	*c = b >> 5;
	s = b & 31;
	lo = M << s;                         /* T = M << s = hi * 2^64 + lo */
	hi = (M >> 32) >> (32 - s);          /* (32 - s is 1..32: no shift by 64) */
	d[0] = lo & 0xffffffffULL;
	d[1] = lo >> 32;
	d[2] = hi;
	*neg = (int)(bits >> 63);
	return 1;
}

static void xsum_add_digits(pft_xsum * a, int c, const uint64_t d[3], int neg)
{
	int j;
	for(j=0;j<3;j++) a->w[c+j] += neg ? -(long long)d[j] : (long long)d[j];
}

int pft_xsum_add(pft_xsum * acc, double x)
{
	uint64_t d[3];
	int c, neg, k;
	if(!acc) return -2;
	k = xsum_digits(x, &c, d, &neg);
	if(k < 0) return -2;
	if(k) xsum_add_digits(acc, c, d, neg);
	return 0;
}

int pft_xsum_combine(pft_xsum * into, const pft_xsum * other)
{
	int j;
	if(!into || !other) return -2;
	/* (unsigned: the words of records within the cell limit cannot overflow, others wrap) */
	for(j=0;j<PFT_XSUM_WORDS;j++) into->w[j] = (long long)((uint64_t)into->w[j] + (uint64_t)other->w[j]);
	return 0;
}

#define XDIGITS (PFT_XSUM_WORDS + 2)   /* the words' carries end in two more 32-bit digits */

/* the carry-propagated digits of sign * acc; returns the final carry (0 when sign * acc >= 0 and
   -1 when it is negative) */
static int xsum_normalise(const pft_xsum * acc, int negate, uint32_t dig[XDIGITS])
{
	i128 carry = 0;
	int j;
	for(j=0;j<XDIGITS;j++) {
		i128 t = carry;
		if(j < PFT_XSUM_WORDS) t += negate ? -(i128)acc->w[j] : (i128)acc->w[j];
		dig[j] = (uint32_t)((unsigned __int128)t & 0xffffffffu);
		carry = t >> 32;                 /* arithmetic: floor */
	}
	return (int)carry;
}

/* bits [pos, pos + 64) of the digit string (zero past its ends) */
static uint64_t xsum_bits(const uint32_t dig[XDIGITS], int pos)
{
	const int j = pos >> 5, s = pos & 31;
	uint64_t d0 = j < XDIGITS ? dig[j] : 0, d1 = j + 1 < XDIGITS ? dig[j+1] : 0, d2 = j + 2 < XDIGITS ? dig[j+2] : 0;
	uint64_t v = d0 | (d1 << 32);
	if(!s) return v;
	return (v >> s) | (d2 << (64 - s));
}

int pft_xsum_round(const pft_xsum * acc, double * out)
{
	uint32_t dig[XDIGITS];
	uint64_t q;
	int neg = 0, top, m, j;
	double r;
	if(!acc || !out) return -2;
	if(xsum_normalise(acc, 0, dig) < 0) {
		neg = 1;
		xsum_normalise(acc, 1, dig);
	}
	for(top = XDIGITS - 1; top >= 0 && !dig[top]; top--) ;
	if(top < 0) { *out = 0.0; return 0; }
	/* N = the integer of the digits, its highest set bit m: the sum is N * 2^-1074 */
	m = 32*top + 31;
	while(!(dig[top] >> (m & 31))) m--;
	if(m <= 52) {
		/* below 2^53: exact (a subnormal, or the first normal binade) */
		r = ldexp((double)xsum_bits(dig, 0), -1074);
	} else {
		const int low = m - 52;          /* the 53 bits kept are [low, m] */
		int round, sticky = 0;
		q = xsum_bits(dig, low) & ((1ULL << 53) - 1);
		round = (int)(xsum_bits(dig, low - 1) & 1);
		for(j = 0; j < (low - 1) >> 5 && !sticky; j++) sticky = dig[j] != 0;
		if(!sticky && ((low - 1) & 31)) sticky = (dig[(low - 1) >> 5] & ((1u << ((low - 1) & 31)) - 1)) != 0;
		if(round && (sticky || (q & 1))) q++;          /* (2^53 is a double, ldexp takes it as it is) */
		r = ldexp((double)q, low - 1074);               /* exact, or +Inf past DBL_MAX */
	}
	*out = neg ? -r : r;
	return 0;
}

int pft_means_combine(pft_means * into, const pft_means * other)
{
	int q;
	if(!into || !other) return -2;
	for(q=0;q<PFT_MEAN_COUNT;q++) {
		into->n[q] += other->n[q];
		pft_xsum_combine(&into->sum[q], &other->sum[q]);
	}
	return 0;
}

int pft_means_host(const pft_grid * g, const double * x, const pft_diag_opts * opts, pft_means * total,
                   pft_means * per_plane)
{
	const int B = PFT_BCOND_THICKNESS;
	double p_thr = 0.5, gl_thr = 0.5;
	long N1, row, S;
	int k;
	if(!g || !x || !total || g->n1 < 1 || g->n2 < 1 || g->n3 < 1) return -2;
	if((long long)g->n1 * g->n2 * g->n3 > 0x7fffffffLL) return -2;
	if(opts) { p_thr = opts->p_thr; gl_thr = opts->gl_thr; }
	N1 = g->n1 + 2L*B; row = N1*(g->n2 + 2L*B); S = row*(g->n3 + 2L*B);
	memset(total, 0, sizeof *total);
	#pragma omp parallel
	{
		pft_means t, m;
		memset(&t, 0, sizeof t);
		#pragma omp for schedule(static) nowait
		for(k=0;k<g->n3;k++) {
			int j, i;
			memset(&m, 0, sizeof m);
			for(j=0;j<g->n2;j++) {
				const double * u = x + PFT_VAR_U*S + (k+B)*row + (long)(j+B)*N1 + B;
				const double * p = u + (PFT_VAR_P - PFT_VAR_U)*S;
				const double * gl = u + (PFT_VAR_GL - PFT_VAR_U)*S;
				for(i=0;i<g->n1;i++) {
					const int ice = p[i] > p_thr, pore = gl[i] < gl_thr;   /* ordered: false on NaN */
					uint64_t d[3];
					int c, neg, kind;
					if((kind = xsum_digits(u[i], &c, d, &neg)) >= 0) {
						m.n[PFT_MEAN_U]++;
						m.n[PFT_MEAN_U_ICE] += ice;
						if(kind) {
							xsum_add_digits(&m.sum[PFT_MEAN_U], c, d, neg);
							if(ice) xsum_add_digits(&m.sum[PFT_MEAN_U_ICE], c, d, neg);
						}
					}
					if((kind = xsum_digits(p[i], &c, d, &neg)) >= 0) {
						m.n[PFT_MEAN_P]++;
						m.n[PFT_MEAN_P_PORE] += pore;
						if(kind) {
							xsum_add_digits(&m.sum[PFT_MEAN_P], c, d, neg);
							if(pore) xsum_add_digits(&m.sum[PFT_MEAN_P_PORE], c, d, neg);
						}
					}
				}
			}
			if(per_plane) per_plane[k] = m;
			pft_means_combine(&t, &m);
		}
		#pragma omp critical(pft_means_merge)
		pft_means_combine(total, &t);
	}
	return 0;
}
