/*
 * pft_formula_selftest.c -- a stand-alone host program over pft_formula.c (with the evaluator of
 * pft_frontend.c and the accumulator of pft_means.c) for runs under the host sanitizers (make -C
 * porousfreezethaw_amd formula-selftest: -fsanitize=address,undefined; no GPU, no Python): the
 * record's combine laws and neutral element, pft_formula_host on a small padded array with
 * poisoned ghosts against sums known without a second implementation, the limits and refusals,
 * the compile rule for C and P, and 1 thread against 4 word for word.  Exit status 0 when every
 * case holds, 1 otherwise.  The comparison against the Python evaluator is
 * tests/test_formula_host.py.
 */
#include "../../include/pft_formula.h"

#include <math.h>
#include <omp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;

#define CHECK(cond, what) do { if(!(cond)) { printf("FAIL %s (line %d)\n", what, __LINE__); failures++; } } while(0)

static int same(const pft_fdiag * a, const pft_fdiag * b) { return memcmp(a, b, sizeof *a) == 0; }

static pft_fdiag comb(const pft_fdiag * a, const pft_fdiag * b)
{
	pft_fdiag r = *a;
	if(pft_fdiag_combine(&r, b)) failures++;
	return r;
}

int main(void)
{
	const int n1 = 5, n2 = 3, n3 = 4, B = PFT_BCOND_THICKNESS;
	const long N1 = n1 + 2*B, row = N1*(n2 + 2*B), S = row*(n3 + 2*B);
	double * x = (double *)malloc(sizeof(double)*3*S);
	pft_grid g;
	pft_fdiag total[PFT_FORMULA_MAX + 1], planes[3*4], again[3], again_planes[3*4], empty, m;
	/* three programs: u;  (p > 0.5) * u;  sqrt(u - 300) / (1 - gl)   [inputs 6 u, 7 p, 8 gl] */
	const int lens[3] = { 1, 5, 9 };
	const int ops[15] = { 101,  101, 100, 12, 101, 3,  101, 100, 1, 41, 100, 101, 1, 4, 21 };
	const double args[15] = { 6,  7, 0.5, 0, 6, 0,  6, 300, 0, 0, 1, 8, 0, 0, 0 };
	double s_all = 0.0, s_ice = 0.0, got;
	long c, k, j, q;
	int f, i, cells = n1*n2*n3;

	omp_set_num_threads(4);
	memset(&g, 0, sizeof g);
	g.n1 = n1; g.n2 = n2; g.n3 = n3; g.total_n3 = n3; g.nprocs = 1; g.L1 = 0.03; g.L2 = 0.03; g.L3 = 0.06;
	/* ghosts: NaN (u), 1 (p), 1 (gl: a division by zero in program 2) */
	for(c=0;c<S;c++) { x[PFT_VAR_U*S + c] = NAN; x[PFT_VAR_P*S + c] = 1.0; x[PFT_VAR_GL*S + c] = 1.0; }
	for(k=0;k<n3;k++) for(j=0;j<n2;j++) for(q=0;q<n1;q++) {
		const long at = (k+B)*row + (j+B)*N1 + q + B;
		const double u = 273.0 + (double)((k*n2 + j)*n1 + q);       /* 273 .. 332: 32 cells above 300 */
		x[PFT_VAR_U*S + at] = u;
		x[PFT_VAR_P*S + at] = k == 2 ? 1.0 : 0.0;
		x[PFT_VAR_GL*S + at] = k == 1 ? 1.0 : 0.0;                   /* plane 1: 1 - gl = 0, a math error */
		s_all += u;
		if(k == 2) s_ice += u;
	}

	/* the neutral element and the combine laws */
	pft_fdiag_init(&empty);
	CHECK(empty.cells == 0 && empty.n == 0 && isinf(empty.min) && empty.min > 0 && isinf(empty.max) && empty.max < 0
	      && empty.maxabs == 0.0, "the record of no cells");
	CHECK(pft_formula_host(&g, x, 3, lens, ops, args, total, planes) == 0, "pft_formula_host");
	for(f=0;f<3;f++) {
		CHECK(same(&(pft_fdiag){0}, &total[f]) == 0, "a record is not zero");
		m = comb(&total[f], &empty); CHECK(same(&m, &total[f]), "neutral on the right");
		m = comb(&empty, &total[f]); CHECK(same(&m, &total[f]), "neutral on the left");
		m = empty;
		for(k=0;k<n3;k++) pft_fdiag_combine(&m, &planes[f*n3 + k]);
		CHECK(same(&m, &total[f]), "the planes combine to the total");
		m = empty;
		for(k=n3-1;k>=0;k--) pft_fdiag_combine(&m, &planes[f*n3 + k]);
		CHECK(same(&m, &total[f]), "... in any order");
	}
	for(i=0;i<12;i++) for(j=0;j<12;j++) {
		pft_fdiag ab = comb(&planes[i], &planes[j]), ba = comb(&planes[j], &planes[i]);
		CHECK(same(&ab, &ba), "commutative");
		for(k=0;k<12;k+=5) {
			pft_fdiag l = comb(&ab, &planes[k]), bc = comb(&planes[j], &planes[k]), r = comb(&planes[i], &bc);
			CHECK(same(&l, &r), "associative");
		}
	}
	{
		pft_fdiag lo = empty, hi = empty;
		lo.cells = lo.n = hi.cells = hi.n = 1;
		lo.min = lo.max = -0.0; hi.min = hi.max = 0.0;
		m = comb(&lo, &hi); CHECK(signbit(m.min) && !signbit(m.max), "-0.0 < +0.0");
		m = comb(&hi, &lo); CHECK(signbit(m.min) && !signbit(m.max), "-0.0 < +0.0, the other way");
	}

	/* the values: no ghost is read */
	CHECK(total[0].cells == cells && total[0].n == cells && total[0].nonzero == cells && total[0].nonfinite == 0, "u: counts");
	CHECK(total[0].min == 273.0 && total[0].max == 332.0 && total[0].maxabs == 332.0, "u: extrema");
	pft_xsum_round(&total[0].sum, &got); CHECK(got == s_all, "u: sum");
	CHECK(total[1].n == cells && total[1].nonzero == n1*n2 && total[1].min == 0.0 && total[1].max == 317.0, "ice u: counts, extrema");
	pft_xsum_round(&total[1].sum, &got); CHECK(got == s_ice, "ice u: sum");
	/* sqrt(u - 300) / (1 - gl): 0 below 300 (planes 0 and most of 1), 0 in plane 1 (1/0), sqrt elsewhere */
	CHECK(total[2].n == cells && total[2].nonfinite == 0 && total[2].min == 0.0, "math errors yield a finite 0");
	CHECK(total[2].nonzero == 2*n1*n2 && planes[2*n3 + 1].nonzero == 0 && total[2].max == sqrt(32.0), "math errors: where");
	CHECK(planes[0*n3 + 3].min == 318.0 && planes[0*n3 + 3].cells == n1*n2, "plane records");

	/* 1 thread against 4, word for word */
	omp_set_num_threads(1);
	CHECK(pft_formula_host(&g, x, 3, lens, ops, args, again, again_planes) == 0, "1 thread");
	CHECK(memcmp(again, total, sizeof again) == 0 && memcmp(again_planes, planes, sizeof planes) == 0, "1 thread == 4 threads");
	omp_set_num_threads(4);

	/* limits and refusals */
	{
		int many_lens[PFT_FORMULA_MAX + 1], many_ops[PFT_FORMULA_MAX_ENTRIES + 2];
		double many_args[PFT_FORMULA_MAX_ENTRIES + 2];
		pft_grid huge = g;
		pft_ic_prog pr;
		const int bad_op[2] = { 101, 16 }, under[1] = { 2 }, two[2] = { 100, 100 }, input9[1] = { 101 };
		const double a9[2] = { 9, 9 };
		for(i=0;i<=PFT_FORMULA_MAX;i++) many_lens[i] = 1;
		for(i=0;i<PFT_FORMULA_MAX_ENTRIES + 2;i++) { many_ops[i] = 100; many_args[i] = 1.0; }
		CHECK(pft_formula_host(&g, x, PFT_FORMULA_MAX, many_lens, many_ops, many_args, total, NULL) == 0, "8 programs");
		CHECK(pft_formula_host(&g, x, PFT_FORMULA_MAX + 1, many_lens, many_ops, many_args, total, NULL) == -2, "9 programs");
		CHECK(pft_formula_host(&g, x, 0, many_lens, many_ops, many_args, total, NULL) == -2, "no program");
		/* 1, then (1 +) 127 times: 255 entries, and one more program of 1: 256 in all */
		for(i=1;i<255;i+=2) many_ops[i+1] = 2;
		many_lens[0] = 255; many_lens[1] = 1;
		CHECK(pft_formula_host(&g, x, 2, many_lens, many_ops, many_args, total, NULL) == 0 && total[0].max == 128.0, "256 entries");
		many_lens[1] = 2;
		CHECK(pft_formula_host(&g, x, 2, many_lens, many_ops, many_args, total, NULL) == -2, "257 entries");
		many_lens[0] = 2;
		CHECK(pft_formula_host(&g, x, 1, many_lens, bad_op, a9, total, NULL) == -2, "an unknown operator");
		many_lens[0] = 1;
		CHECK(pft_formula_host(&g, x, 1, many_lens, under, a9, total, NULL) == -2, "a stack underflow");
		CHECK(pft_formula_host(&g, x, 1, many_lens, input9, a9, total, NULL) == -2, "an input past gl");
		many_lens[0] = 2;
		CHECK(pft_formula_host(&g, x, 1, many_lens, two, a9, total, NULL) == -2, "two values left");
		huge.n1 = 2048; huge.n2 = 1024; huge.n3 = huge.total_n3 = 1024;
		many_lens[0] = 1;
		CHECK(pft_formula_host(&huge, x, 1, many_lens, many_ops, many_args, total, NULL) == -2, "2^31 cells");
		CHECK(pft_formula_host(&g, NULL, 1, many_lens, many_ops, many_args, total, NULL) == -2
		      && pft_formula_host(&g, x, 1, many_lens, many_ops, many_args, NULL, NULL) == -2
		      && pft_fdiag_combine(NULL, &empty) == -2 && pft_fdiag_combine(&m, NULL) == -2, "NULL");
		/* the compile rule: u C 2 is not device-exact, 5 C 2 + u folds, the second program above compiles */
		{
			const int uc2[3] = { 101, 100, 5 }, c52[5] = { 100, 100, 5, 101, 2 };
			const double uc2a[3] = { 6, 2, 0 }, c52a[5] = { 5, 2, 0, 6, 0 };
			CHECK(pft_formula_compile(&g, 3, uc2, uc2a, &pr) == 1, "u C 2 stays on the host");
			CHECK(pft_formula_compile(&g, 5, c52, c52a, &pr) == 0 && pr.n == 3 && pr.arg[0] == 10.0, "5 C 2 + u folds");
			pft_ic_prog_free(&pr);
			CHECK(pft_formula_compile(&g, 5, ops + 1, args + 1, &pr) == 0, "(p > 0.5) * u compiles");
			pft_ic_prog_free(&pr);
			CHECK(pft_formula_compile(&g, PFT_FORMULA_MAX_ENTRIES + 1, many_ops, many_args, &pr) == -2, "a program too long");
		}
	}
	free(x);
	printf(failures ? "pft_formula_selftest: %d FAILED\n" : "pft_formula_selftest: ok\n", failures);
	return failures ? 1 : 0;
}
