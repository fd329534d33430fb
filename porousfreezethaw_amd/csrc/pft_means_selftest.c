/*
 * pft_means_selftest.c -- a stand-alone host program over pft_means.c for runs under the host
 * sanitizers (make -C porousfreezethaw_amd means-selftest: -fsanitize=address,undefined; no GPU, no
 * Python): the add / combine / round cases whose results are known without a second
 * implementation, and pft_means_host on a small padded array with poisoned ghosts.  Exit status 0
 * when every case holds, 1 otherwise.  The comparison against exact rational arithmetic is
 * tests/test_means_host.py.
 */
#include "../../include/pft_means.h"

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;

static int same(double a, double b)
{
	return memcmp(&a, &b, 8) == 0;
}

static void expect_sum(const char * what, const double * v, int n, double want)
{
	pft_xsum acc, half[2], rev;
	double got = -1.0, got2 = -1.0, got3 = -1.0;
	int i;
	memset(&acc, 0, sizeof acc); memset(half, 0, sizeof half); memset(&rev, 0, sizeof rev);
	for(i=0;i<n;i++) {
		if(pft_xsum_add(&acc, v[i]) || pft_xsum_add(&half[i & 1], v[i]) || pft_xsum_add(&rev, v[n-1-i])) failures++;
	}
	pft_xsum_combine(&half[0], &half[1]);
	if(pft_xsum_round(&acc, &got) || pft_xsum_round(&half[0], &got2) || pft_xsum_round(&rev, &got3)) failures++;
	if(memcmp(&acc, &half[0], sizeof acc) || memcmp(&acc, &rev, sizeof acc)) { printf("FAIL %s: words depend on the order\n", what); failures++; }
	if(!same(got, want) || !same(got2, want) || !same(got3, want)) { printf("FAIL %s: %a, want %a\n", what, got, want); failures++; }
}

#define SUM(what, want, ...) do { const double v_[] = { __VA_ARGS__ }; \
	expect_sum(what, v_, (int)(sizeof v_ / sizeof v_[0]), want); } while(0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t rng(void)
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return rng_state;
}

int main(void)
{
	const double two53 = 9007199254740992.0, tiny = 4.9406564584124654e-324, half_ulp_max = ldexp(1.0, 970);
	double v[4096], out;
	pft_xsum z;
	int i, n;

	SUM("one value", 273.15, 273.15);
	SUM("nothing", 0.0, 0.0, -0.0);
	SUM("exact zero is +0", 0.0, 1.5, -1.5);
	SUM("DBL_MAX cancels", 0.0, DBL_MAX, -DBL_MAX);
	SUM("DBL_MAX survives", DBL_MAX, DBL_MAX, DBL_MAX, -DBL_MAX);
	SUM("overflow", INFINITY, DBL_MAX, DBL_MAX);
	SUM("negative overflow", -INFINITY, -DBL_MAX, -DBL_MAX);
	SUM("tie at DBL_MAX goes to the even 2^1024", INFINITY, DBL_MAX, half_ulp_max);
	SUM("below that tie", DBL_MAX, DBL_MAX, nextafter(half_ulp_max, 0.0));
	SUM("tie down to even", two53, two53, 1.0);
	SUM("tie up to even", two53 + 4.0, two53 + 2.0, 1.0);
	SUM("sticky bit breaks the tie", two53 + 2.0, two53, 1.0, tiny);
	SUM("negative tie", -two53, -two53, -1.0);
	SUM("carry into the next binade", ldexp(1.0, 54), ldexp(1.0, 54) - 2.0, 1.0);
	SUM("cancels to a subnormal", 3*tiny, 1.0, 3*tiny, -1.0);
	SUM("huge cancels to a subnormal", -2.5e-310, 1e308, -2.5e-310, -1e308);
	SUM("subnormals", 7*tiny, tiny, 2*tiny, 4*tiny);
	SUM("below the first normal", DBL_MIN - tiny, DBL_MIN, -tiny);

	/* integers below 2^40 of both signs: the sum is exact in 64-bit integers and in double */
	for(n = 1; n <= 4096; n *= 4) {
		long long total = 0;
		for(i=0;i<n;i++) {
			long long k = (long long)(rng() >> 24) - (1LL << 39);
			v[i] = (double)k;
			total += k;
		}
		expect_sum("integers", v, n, (double)total + 0.0);
	}
	/* x and -x over every exponent, shuffled by the generator: exactly zero */
	for(i=0;i<2048;i+=2) {
		uint64_t bits = (rng() & 0x800fffffffffffffULL) | ((uint64_t)(i % 2047) << 52);
		memcpy(&v[i], &bits, 8);
		if(!isfinite(v[i])) v[i] = 1.0;
		v[i+1] = -v[i];
	}
	expect_sum("x and -x over every exponent", v, 2048, 0.0);

	memset(&z, 0, sizeof z);
	if(pft_xsum_add(&z, NAN) != -2 || pft_xsum_add(&z, INFINITY) != -2 || pft_xsum_add(NULL, 1.0) != -2
	   || pft_xsum_round(&z, NULL) != -2 || pft_xsum_combine(NULL, &z) != -2) { printf("FAIL refusals\n"); failures++; }
	for(i=0;i<PFT_XSUM_WORDS;i++) if(z.w[i]) { printf("FAIL a refused value was added\n"); failures++; break; }
	/* any words are accepted: the extremes of every word */
	for(i=0;i<PFT_XSUM_WORDS;i++) z.w[i] = (i & 1) ? INT64_MAX : INT64_MIN;
	if(pft_xsum_round(&z, &out) || !isinf(out)) { printf("FAIL extreme words\n"); failures++; }
	pft_xsum_combine(&z, &z);

	/* pft_means_host: 5x3x4 cells, u = 273 + cell index, p = 1 in plane 2 only, gl = 0 in plane 1
	   only; ghosts hold NaN (u), 1 (p) and -1 (gl) */
	{
		pft_grid g;
		const int n1 = 5, n2 = 3, n3 = 4, B = PFT_BCOND_THICKNESS;
		const long N1 = n1 + 2*B, row = N1*(n2 + 2*B), S = row*(n3 + 2*B);
		double * x = (double *)malloc(sizeof(double)*3*S);
		pft_means total, planes[4], merged;
		double s_all = 0.0, s_ice = 0.0, got;
		long c, k, j, q;
		memset(&g, 0, sizeof g);
		g.n1 = n1; g.n2 = n2; g.n3 = n3; g.total_n3 = n3; g.nprocs = 1;
		for(c=0;c<S;c++) { x[PFT_VAR_U*S + c] = NAN; x[PFT_VAR_P*S + c] = 1.0; x[PFT_VAR_GL*S + c] = -1.0; }
		for(k=0;k<n3;k++) for(j=0;j<n2;j++) for(q=0;q<n1;q++) {
			const long at = (k+B)*row + (j+B)*N1 + q + B;
			const double u = 273.0 + (double)((k*n2 + j)*n1 + q);
			x[PFT_VAR_U*S + at] = u;
			x[PFT_VAR_P*S + at] = k == 2 ? 1.0 : 0.0;
			x[PFT_VAR_GL*S + at] = k == 1 ? 0.0 : 1.0;
			s_all += u;
			if(k == 2) s_ice += u;
		}
		if(pft_means_host(&g, x, NULL, &total, planes)) { printf("FAIL pft_means_host\n"); failures++; }
		if(total.n[PFT_MEAN_U] != 60 || total.n[PFT_MEAN_P] != 60 || total.n[PFT_MEAN_U_ICE] != 15
		   || total.n[PFT_MEAN_P_PORE] != 15) { printf("FAIL counts\n"); failures++; }
		pft_xsum_round(&total.sum[PFT_MEAN_U], &got);
		if(!same(got, s_all)) { printf("FAIL sum u %a\n", got); failures++; }
		pft_xsum_round(&total.sum[PFT_MEAN_U_ICE], &got);
		if(!same(got, s_ice)) { printf("FAIL sum ice u %a\n", got); failures++; }
		pft_xsum_round(&total.sum[PFT_MEAN_P], &got);
		if(!same(got, 15.0)) { printf("FAIL sum p %a\n", got); failures++; }
		pft_xsum_round(&total.sum[PFT_MEAN_P_PORE], &got);
		if(!same(got, 0.0)) { printf("FAIL sum pore p %a\n", got); failures++; }
		memset(&merged, 0, sizeof merged);
		for(k=0;k<n3;k++) pft_means_combine(&merged, &planes[k]);
		if(memcmp(&merged, &total, sizeof total)) { printf("FAIL the planes do not add up\n"); failures++; }
		if(pft_means_host(&g, x, NULL, NULL, NULL) != -2 || pft_means_combine(NULL, &total) != -2) { printf("FAIL refusals (means)\n"); failures++; }
		free(x);
	}
	printf(failures ? "pft_means_selftest: %d FAILED\n" : "pft_means_selftest: ok\n", failures);
	return failures ? 1 : 0;
}
