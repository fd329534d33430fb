/*
 * pft_hist_selftest.c -- a stand-alone host program over pft_hist.c (with the evaluator of
 * pft_frontend.c) for runs under the host sanitizers (make -C porousfreezethaw_amd hist-selftest:
 * -fsanitize=address,undefined; no GPU, no Python): the bin rule on its edge cases, the combine
 * laws, pft_hist_host on a small padded array with poisoned ghosts against counts known without a
 * second implementation, a guard word behind every output array, 1 and 1024 bins, every refusal,
 * and 1 thread against 4 word for word.  Exit status 0 when every case holds, 1 otherwise.  The
 * comparison against numpy.histogram is tests/test_hist_host.py.
 */
#include "../../include/pft_hist.h"

#include <math.h>
#include <omp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;

#define CHECK(cond, what) do { if(!(cond)) { printf("FAIL %s (line %d)\n", what, __LINE__); failures++; } } while(0)
#define GUARD 0x5a5a5a5a5a5a5a5aLL

int main(void)
{
	const int n1 = 5, n2 = 3, n3 = 4, B = PFT_BCOND_THICKNESS;
	const long N1 = n1 + 2*B, row = N1*(n2 + 2*B), S = row*(n3 + 2*B);
	const int cells = n1*n2*n3;
	double * x = (double *)malloc(sizeof(double)*3*S);
	pft_grid g;
	/* u;  p > 0.5;  1 / (gl - gl)   [inputs 6 u, 7 p, 8 gl] */
	const int u_op[1] = { 101 }, ice_op[3] = { 101, 100, 12 }, err_op[5] = { 100, 101, 101, 1, 4 };
	const double u_arg[1] = { 6 }, ice_arg[3] = { 7, 0.5, 0 }, err_arg[5] = { 1, 8, 8, 0, 0 };
	const pft_hist_prog pu = { 1, u_op, u_arg }, pice = { 3, ice_op, ice_arg }, perr = { 5, err_op, err_arg };
	const pft_hist_prog pp = { 1, u_op, ice_arg };       /* p itself: input 7 */
	const double e4[5] = { 273.0, 280.0, 300.0, 320.0, 332.0 };     /* the last edge is the largest u */
	const double e0[4] = { -1.0, 0.0, 5e-324, 1.0 };
	pft_hist_head h, h4, ph[4 + 1], again_h, again_ph[4];
	long long c4[4 + 1], pc[4*4 + 1], again_c[4], again_pc[16], * big, * bigp;
	double * e1024;
	long c, k, j, q;
	int i, b;

	omp_set_num_threads(4);
	memset(&g, 0, sizeof g);
	g.n1 = n1; g.n2 = n2; g.n3 = n3; g.total_n3 = n3; g.nprocs = 1; g.L1 = 0.03; g.L2 = 0.03; g.L3 = 0.06;
	/* ghosts: NaN (u), 1 (p: ice), 1 (gl) -- any of them counted would change the counts below */
	for(c=0;c<S;c++) { x[PFT_VAR_U*S + c] = NAN; x[PFT_VAR_P*S + c] = 1.0; x[PFT_VAR_GL*S + c] = 1.0; }
	for(k=0;k<n3;k++) for(j=0;j<n2;j++) for(q=0;q<n1;q++) {
		const long at = (k+B)*row + (j+B)*N1 + q + B;
		x[PFT_VAR_U*S + at] = 273.0 + (double)((k*n2 + j)*n1 + q);      /* 273 .. 332, one each */
		x[PFT_VAR_P*S + at] = k == 2 ? 1.0 : (k == 3 ? NAN : 0.0);     /* plane 2 ice, plane 3 a NaN mask */
		x[PFT_VAR_GL*S + at] = 0.0;
	}

	/* the bin rule on its edge cases */
	CHECK(pft_hist_bin(3, e0, 0.0) == 1 && pft_hist_bin(3, e0, -0.0) == 1, "+-0.0 on an edge at 0.0");
	CHECK(pft_hist_bin(3, e0, -5e-324) == 0 && pft_hist_bin(3, e0, 5e-324) == 2, "both neighbours of 0.0");
	CHECK(pft_hist_bin(3, e0, -1.0) == 0 && pft_hist_bin(3, e0, 1.0) == 2, "the first and the last edge");
	CHECK(pft_hist_bin(3, e0, nextafter(-1.0, -2.0)) == PFT_HIST_UNDER && pft_hist_bin(3, e0, nextafter(1.0, 2.0)) == PFT_HIST_OVER,
	      "the outer neighbours of the outer edges");
	CHECK(pft_hist_bin(3, e0, nextafter(1.0, 0.0)) == 2 && pft_hist_bin(3, e0, nextafter(-1.0, 0.0)) == 0, "the inner ones");
	CHECK(pft_hist_bin(3, e0, -INFINITY) == PFT_HIST_UNDER && pft_hist_bin(3, e0, INFINITY) == PFT_HIST_OVER
	      && pft_hist_bin(3, e0, NAN) == PFT_HIST_NAN, "-Inf, +Inf, NaN");
	CHECK(pft_hist_bin(1, e0, -1.0) == 0 && pft_hist_bin(1, e0, 0.0) == 0 && pft_hist_bin(1, e0, -0.5) == 0, "one bin");

	/* every refusal of the judge */
	{
		const double nan_e[2] = { 0.0, NAN }, inf_e[2] = { 0.0, INFINITY }, ninf_e[2] = { -INFINITY, 0.0 }, eq[3] = { 0.0, 1.0, 1.0 },
		             zz[2] = { -0.0, 0.0 }, zz2[2] = { 0.0, -0.0 }, down[2] = { 1.0, 0.0 };
		CHECK(pft_hist_check(4, e4) == 0 && pft_hist_check(3, e0) == 0, "good edges");
		CHECK(pft_hist_check(0, e4) == -2 && pft_hist_check(PFT_HIST_MAX_BINS + 1, e4) == -2 && pft_hist_check(4, NULL) == -2,
		      "nbins and NULL");
		CHECK(pft_hist_check(1, nan_e) == -2 && pft_hist_check(1, inf_e) == -2 && pft_hist_check(1, ninf_e) == -2, "NaN, +-Inf");
		CHECK(pft_hist_check(2, eq) == -2 && pft_hist_check(1, zz) == -2 && pft_hist_check(1, zz2) == -2 && pft_hist_check(1, down) == -2,
		      "equal neighbours, -0.0 next to +0.0, decreasing");
	}

	/* the host twin: counts known from the layout, guards behind every output array */
	c4[4] = GUARD; pc[16] = GUARD; ph[4].cells = GUARD;
	CHECK(pft_hist_host(&g, x, &pu, NULL, 4, e4, &h4, c4, ph, pc) == 0, "pft_hist_host");
	CHECK(h4.cells == cells && h4.selected == cells && h4.nan == 0 && h4.under == 0 && h4.over == 0, "the head without a mask");
	CHECK(c4[0] == 7 && c4[1] == 20 && c4[2] == 20 && c4[3] == 13, "the counts: 332 belongs to the last bin");
	CHECK(c4[4] == GUARD && pc[16] == GUARD && ph[4].cells == GUARD, "the guards");
	{
		pft_hist_head sum; long long sc[4];
		memset(&sum, 0, sizeof sum); memset(sc, 0, sizeof sc);
		for(k=0;k<n3;k++) CHECK(pft_hist_combine(4, &sum, sc, &ph[k], pc + 4*k) == 0, "combine");
		CHECK(memcmp(&sum, &h4, sizeof sum) == 0 && memcmp(sc, c4, sizeof sc) == 0, "the planes combine to the total");
		CHECK(ph[0].cells == n1*n2 && pc[0] == 7 && pc[1] == 8 && pc[4*3 + 3] == 13, "plane rows");
	}
	/* the mask p > 0.5: plane 2 (a NaN p is not > 0.5); the mask p: planes 2 and 3 (a NaN selects) */
	CHECK(pft_hist_host(&g, x, &pu, &pice, 4, e4, &h, c4, NULL, NULL) == 0 && h.selected == 15 && h.cells == cells
	      && c4[0] + c4[1] + c4[2] + c4[3] == 15 && c4[2] == 15, "mask p > 0.5");
	CHECK(pft_hist_host(&g, x, &pu, &pp, 4, e4, &h, c4, NULL, NULL) == 0 && h.selected == 30 && c4[2] == 17 && c4[3] == 13, "a NaN mask selects");
	CHECK(pft_hist_host(&g, x, &pu, &perr, 4, e4, &h, c4, NULL, NULL) == 0 && h.selected == 0 && c4[0] + c4[1] + c4[2] + c4[3] == 0,
	      "a math error in the mask does not");
	CHECK(pft_hist_host(&g, x, &perr, NULL, 3, e0, &h, c4, NULL, NULL) == 0 && h.selected == cells && c4[1] == cells, "... in the value: 0");
	/* p as the value: 30 zeros and ones, 15 NaN; narrow edges: under and over */
	CHECK(pft_hist_host(&g, x, &pp, NULL, 3, e0, &h, c4, NULL, NULL) == 0 && h.nan == 15 && c4[1] == 30 && c4[2] == 15
	      && h.selected == h.nan + h.under + h.over + c4[0] + c4[1] + c4[2], "NaN values and the invariant");
	CHECK(pft_hist_host(&g, x, &pu, NULL, 1, e4 + 1, &h, c4, NULL, NULL) == 0 && h.under == 7 && h.over == 32 && c4[0] == 21,
	      "one bin [280, 300]: under, over");

	/* 1024 bins */
	e1024 = (double *)malloc(sizeof(double)*(PFT_HIST_MAX_BINS + 1));
	big = (long long *)malloc(sizeof(long long)*(PFT_HIST_MAX_BINS + 1));
	bigp = (long long *)malloc(sizeof(long long)*((size_t)n3*PFT_HIST_MAX_BINS + 1));
	for(i=0;i<=PFT_HIST_MAX_BINS;i++) e1024[i] = 273.0 + i * (59.0 / 1024.0) * 1.0;
	e1024[PFT_HIST_MAX_BINS] = 332.0;
	big[PFT_HIST_MAX_BINS] = GUARD; bigp[(size_t)n3*PFT_HIST_MAX_BINS] = GUARD;
	CHECK(pft_hist_check(PFT_HIST_MAX_BINS, e1024) == 0, "1024 bins: edges");
	CHECK(pft_hist_host(&g, x, &pu, NULL, PFT_HIST_MAX_BINS, e1024, &h, big, ph, bigp) == 0, "1024 bins");
	{
		long long all = 0, planes = 0;
		for(b=0;b<PFT_HIST_MAX_BINS;b++) { all += big[b]; CHECK(big[b] == 0 || big[b] == 1, "one value per bin at most"); }
		for(c=0;c<(long)n3*PFT_HIST_MAX_BINS;c++) planes += bigp[c];
		CHECK(all == cells && planes == cells && big[0] == 1 && big[PFT_HIST_MAX_BINS - 1] == 1, "1024 bins: every cell once");
		CHECK(big[PFT_HIST_MAX_BINS] == GUARD && bigp[(size_t)n3*PFT_HIST_MAX_BINS] == GUARD, "1024 bins: the guards");
	}

	/* the combine laws */
	{
		pft_hist_head a = ph[0], bb = ph[1], zero, ab, ba, l, r;
		long long ca[4], cb[4], cz[4], cab[4], cba[4], cl[4], cr[4];
		memset(&zero, 0, sizeof zero); memset(cz, 0, sizeof cz);
		memcpy(ca, pc, sizeof ca); memcpy(cb, pc + 4, sizeof cb);
		ab = a; memcpy(cab, ca, sizeof ca); pft_hist_combine(4, &ab, cab, &bb, cb);
		ba = bb; memcpy(cba, cb, sizeof cb); pft_hist_combine(4, &ba, cba, &a, ca);
		CHECK(memcmp(&ab, &ba, sizeof ab) == 0 && memcmp(cab, cba, sizeof cab) == 0, "commutative");
		l = ab; memcpy(cl, cab, sizeof cl); pft_hist_combine(4, &l, cl, &ph[2], pc + 8);
		r = bb; memcpy(cr, cb, sizeof cr); pft_hist_combine(4, &r, cr, &ph[2], pc + 8);
		{ pft_hist_head t = a; long long ct[4]; memcpy(ct, ca, sizeof ct); pft_hist_combine(4, &t, ct, &r, cr); r = t; memcpy(cr, ct, sizeof cr); }
		CHECK(memcmp(&l, &r, sizeof l) == 0 && memcmp(cl, cr, sizeof cl) == 0, "associative");
		l = a; memcpy(cl, ca, sizeof cl); pft_hist_combine(4, &l, cl, &zero, cz);
		CHECK(memcmp(&l, &a, sizeof l) == 0 && memcmp(cl, ca, sizeof cl) == 0, "the zeroed record is neutral");
		CHECK(pft_hist_combine(4, NULL, ca, &a, ca) == -2 && pft_hist_combine(4, &l, NULL, &a, ca) == -2
		      && pft_hist_combine(4, &l, cl, NULL, ca) == -2 && pft_hist_combine(4, &l, cl, &a, NULL) == -2
		      && pft_hist_combine(0, &l, cl, &a, ca) == -2 && pft_hist_combine(PFT_HIST_MAX_BINS + 1, &l, cl, &a, ca) == -2,
		      "combine refuses");
	}

	/* every refusal of the host twin; no refused call writes */
	{
		const int bad_op[1] = { 2 }, in_op[1] = { 101 };
		const double in_arg[1] = { 9 }, down[2] = { 1.0, 0.0 };
		const pft_hist_prog pbad = { 1, bad_op, u_arg }, pin = { 1, in_op, in_arg }, pnone = { 0, u_op, u_arg },
		                    pnull = { 1, NULL, u_arg }, plong = { PFT_FORMULA_MAX_ENTRIES + 1, u_op, u_arg };
		pft_grid none = g, huge = g;
		none.n3 = 0;
		huge.n1 = 2048; huge.n2 = 1024; huge.n3 = 1024;
		h.cells = -77; c4[0] = -77;
		CHECK(pft_hist_host(NULL, x, &pu, NULL, 4, e4, &h, c4, NULL, NULL) == -2 && pft_hist_host(&g, NULL, &pu, NULL, 4, e4, &h, c4, NULL, NULL) == -2
		      && pft_hist_host(&g, x, NULL, NULL, 4, e4, &h, c4, NULL, NULL) == -2 && pft_hist_host(&g, x, &pu, NULL, 4, NULL, &h, c4, NULL, NULL) == -2
		      && pft_hist_host(&g, x, &pu, NULL, 4, e4, NULL, c4, NULL, NULL) == -2 && pft_hist_host(&g, x, &pu, NULL, 4, e4, &h, NULL, NULL, NULL) == -2,
		      "NULL arguments");
		CHECK(pft_hist_host(&g, x, &pbad, NULL, 4, e4, &h, c4, NULL, NULL) == -2 && pft_hist_host(&g, x, &pu, &pbad, 4, e4, &h, c4, NULL, NULL) == -2
		      && pft_hist_host(&g, x, &pin, NULL, 4, e4, &h, c4, NULL, NULL) == -2 && pft_hist_host(&g, x, &pnone, NULL, 4, e4, &h, c4, NULL, NULL) == -2
		      && pft_hist_host(&g, x, &pnull, NULL, 4, e4, &h, c4, NULL, NULL) == -2 && pft_hist_host(&g, x, &plong, NULL, 4, e4, &h, c4, NULL, NULL) == -2,
		      "bad programs");
		CHECK(pft_hist_host(&g, x, &pu, NULL, 0, e4, &h, c4, NULL, NULL) == -2 && pft_hist_host(&g, x, &pu, NULL, PFT_HIST_MAX_BINS + 1, e1024, &h, c4, NULL, NULL) == -2
		      && pft_hist_host(&g, x, &pu, NULL, 1, down, &h, c4, NULL, NULL) == -2, "bad edges");
		CHECK(pft_hist_host(&none, x, &pu, NULL, 4, e4, &h, c4, NULL, NULL) == -2 && pft_hist_host(&huge, x, &pu, NULL, 4, e4, &h, c4, NULL, NULL) == -2,
		      "a grid without cells, with 2^31");
		CHECK(h.cells == -77 && c4[0] == -77, "no refused call writes");
	}

	/* 1 thread against 4, word for word */
	CHECK(pft_hist_host(&g, x, &pu, &pp, 4, e4, &h4, c4, ph, pc) == 0, "4 threads");
	omp_set_num_threads(1);
	CHECK(pft_hist_host(&g, x, &pu, &pp, 4, e4, &again_h, again_c, again_ph, again_pc) == 0, "1 thread");
	CHECK(memcmp(&h4, &again_h, sizeof h4) == 0 && memcmp(c4, again_c, sizeof again_c) == 0
	      && memcmp(ph, again_ph, sizeof again_ph) == 0 && memcmp(pc, again_pc, sizeof again_pc) == 0, "1 thread == 4 threads");

	free(x); free(e1024); free(big); free(bigp);
	if(failures) { printf("pft_hist_selftest: %d failure(s)\n", failures); return 1; }
	printf("pft_hist_selftest: ok\n");
	return 0;
}
