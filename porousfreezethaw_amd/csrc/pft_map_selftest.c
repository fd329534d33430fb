/*
 * pft_map_selftest.c -- a stand-alone host program over pft_map.c (with the evaluator of
 * pft_frontend.c) for runs under the host sanitizers (make -C porousfreezethaw_amd map-selftest:
 * -fsanitize=address,undefined; no GPU, no Python): the neutral record and the combine laws,
 * pft_map_host for every axis on a small padded array with poisoned ghosts against records known
 * without a second implementation, the NaN, +-Inf and signed-zero rules, a guard record behind every
 * output map, slabs of 2 + 1 + 1 planes against one slab, every refusal, and 1 thread against 4 word
 * for word.  Exit status 0 when every case holds, 1 otherwise.  The comparison against numpy is
 * tests/test_map_host.py.
 */
#include "../../include/pft_map.h"

#include <math.h>
#include <omp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;

#define CHECK(cond, what) do { if(!(cond)) { printf("FAIL %s (line %d)\n", what, __LINE__); failures++; } } while(0)
#define GUARD 0x5a5a5a5a5a5a5a5aLL

enum { N1 = 5, N2 = 3, N3 = 4 };

static double * state(int n3, int k0, long * S_out)
{
	/* planes k0 .. k0 + n3 - 1 of the 5 x 3 x 4 state: u = 273 + the cell's global number; p: plane 2
	   ice, plane 3 NaN, else 0; gl 0.  Ghosts: NaN (u), 1 (p), 1 (gl) */
	const int B = PFT_BCOND_THICKNESS;
	const long W = N1 + 2*B, row = W*(N2 + 2*B), S = row*(n3 + 2*B);
	double * x = (double *)malloc(sizeof(double)*3*S);
	long c, k, j, q;
	for(c=0;c<S;c++) { x[PFT_VAR_U*S + c] = NAN; x[PFT_VAR_P*S + c] = 1.0; x[PFT_VAR_GL*S + c] = 1.0; }
	for(k=0;k<n3;k++) for(j=0;j<N2;j++) for(q=0;q<N1;q++) {
		const long at = (k+B)*row + (j+B)*W + q + B, gk = k + k0;
		x[PFT_VAR_U*S + at] = 273.0 + (double)((gk*N2 + j)*N1 + q);
		x[PFT_VAR_P*S + at] = gk == 2 ? 1.0 : (gk == 3 ? NAN : 0.0);
		x[PFT_VAR_GL*S + at] = 0.0;
	}
	*S_out = S;
	return x;
}

static void grid(pft_grid * g, int n3, int first_row)
{
	memset(g, 0, sizeof *g);
	g->n1 = N1; g->n2 = N2; g->n3 = n3; g->total_n3 = N3; g->first_row = first_row; g->nprocs = 1;
	g->L1 = 0.03; g->L2 = 0.03; g->L3 = 0.06;
}

int main(void)
{
	const int B = PFT_BCOND_THICKNESS;
	/* u;  p > 0.5;  p;  1 / (gl - gl)   [inputs 6 u, 7 p, 8 gl] */
	const int u_op[1] = { 101 }, ice_op[3] = { 101, 100, 12 }, err_op[5] = { 100, 101, 101, 1, 4 };
	const double u_arg[1] = { 6 }, ice_arg[3] = { 7, 0.5, 0 }, err_arg[5] = { 1, 8, 8, 0, 0 };
	const pft_hist_prog pu = { 1, u_op, u_arg }, pice = { 3, ice_op, ice_arg }, perr = { 5, err_op, err_arg };
	const pft_hist_prog pp = { 1, u_op, ice_arg };       /* p itself: input 7 */
	pft_grid g;
	pft_map_px m0[N2*N1 + 1], m1[N3*N1 + 1], m2[N3*N2 + 1], again[N3*N1], neutral, t;
	long S, q;
	double * x = state(N3, 0, &S);
	int rows, cols, axis, i, j, k;

	omp_set_num_threads(4);
	grid(&g, N3, 0);

	/* the neutral record, the shapes */
	pft_map_init(&neutral);
	CHECK(sizeof(pft_map_px) == 56, "56 bytes");
	CHECK(neutral.selected == 0 && neutral.nonzero == 0 && neutral.nonfinite == 0 && neutral.min == INFINITY
	      && neutral.max == -INFINITY && neutral.first == -1 && neutral.last == -1, "the neutral record");
	CHECK(pft_map_dims(&g, 0, &rows, &cols) == 0 && rows == N2 && cols == N1, "dims, axis 0");
	CHECK(pft_map_dims(&g, 1, &rows, &cols) == 0 && rows == N3 && cols == N1, "dims, axis 1");
	CHECK(pft_map_dims(&g, 2, &rows, &cols) == 0 && rows == N3 && cols == N2, "dims, axis 2");

	/* u without a mask: every line complete, min and max at its ends, first and last the whole line */
	m0[N2*N1].selected = GUARD; m1[N3*N1].selected = GUARD; m2[N3*N2].selected = GUARD;
	CHECK(pft_map_host(&g, x, &pu, NULL, 0, m0) == 0 && pft_map_host(&g, x, &pu, NULL, 1, m1) == 0
	      && pft_map_host(&g, x, &pu, NULL, 2, m2) == 0, "pft_map_host");
	for(j=0;j<N2;j++) for(i=0;i<N1;i++) {
		const pft_map_px * p = &m0[j*N1 + i];
		CHECK(p->selected == N3 && p->nonzero == N3 && p->nonfinite == 0 && p->first == 0 && p->last == N3 - 1
		      && p->min == 273.0 + j*N1 + i && p->max == 273.0 + (3*N2 + j)*N1 + i, "axis 0: u");
	}
	for(k=0;k<N3;k++) for(i=0;i<N1;i++) {
		const pft_map_px * p = &m1[k*N1 + i];
		CHECK(p->selected == N2 && p->first == 0 && p->last == N2 - 1 && p->min == 273.0 + k*N2*N1 + i
		      && p->max == 273.0 + (k*N2 + 2)*N1 + i, "axis 1: u");
	}
	for(k=0;k<N3;k++) for(j=0;j<N2;j++) {
		const pft_map_px * p = &m2[k*N2 + j];
		CHECK(p->selected == N1 && p->first == 0 && p->last == N1 - 1 && p->min == 273.0 + (k*N2 + j)*N1
		      && p->max == 273.0 + (k*N2 + j)*N1 + 4, "axis 2: u");
	}
	CHECK(m0[N2*N1].selected == GUARD && m1[N3*N1].selected == GUARD && m2[N3*N2].selected == GUARD, "the guards");

	/* p > 0.5 as the value: plane 2 alone is true (a NaN p is not > 0.5) */
	CHECK(pft_map_host(&g, x, &pice, NULL, 0, m0) == 0, "ice, axis 0");
	for(q=0;q<N2*N1;q++)
		CHECK(m0[q].selected == N3 && m0[q].nonzero == 1 && m0[q].first == 2 && m0[q].last == 2 && m0[q].min == 0.0
		      && m0[q].max == 1.0 && m0[q].nonfinite == 0, "axis 0: the ice plane");
	/* p as the value: 0, 0, 1, NaN -- the NaN is "true" (last = 3), nonfinite, and in no extremum */
	CHECK(pft_map_host(&g, x, &pp, NULL, 0, m0) == 0, "p, axis 0");
	for(q=0;q<N2*N1;q++)
		CHECK(m0[q].nonzero == 2 && m0[q].nonfinite == 1 && m0[q].first == 2 && m0[q].last == 3 && m0[q].min == 0.0
		      && m0[q].max == 1.0, "axis 0: a NaN counts as true and wins no extremum");
	/* p as the mask of u: planes 2 and 3 (a NaN selects); p > 0.5: plane 2; a math error: nothing */
	CHECK(pft_map_host(&g, x, &pu, &pp, 0, m0) == 0, "mask p");
	for(q=0;q<N2*N1;q++)
		CHECK(m0[q].selected == 2 && m0[q].first == 2 && m0[q].last == 3 && m0[q].min == 273.0 + 2*N2*N1 + q
		      && m0[q].max == 273.0 + 3*N2*N1 + q, "a NaN mask selects");
	CHECK(pft_map_host(&g, x, &pu, &pice, 1, m1) == 0, "mask p > 0.5, axis 1");
	for(k=0;k<N3;k++) for(i=0;i<N1;i++) {
		t = k == 2 ? m1[k*N1 + i] : neutral;
		CHECK(memcmp(&m1[k*N1 + i], &t, sizeof t) == 0 && (k != 2 || (t.selected == N2 && t.last == N2 - 1)),
		      "rows outside the mask are neutral");
	}
	CHECK(pft_map_host(&g, x, &pu, &perr, 2, m2) == 0, "a math error in the mask");
	for(q=0;q<N3*N2;q++) CHECK(memcmp(&m2[q], &neutral, sizeof neutral) == 0, "a math error in the mask selects nothing");
	CHECK(pft_map_host(&g, x, &perr, NULL, 2, m2) == 0, "a math error in the value");
	for(q=0;q<N3*N2;q++)
		CHECK(m2[q].selected == N1 && m2[q].nonzero == 0 && m2[q].first == -1 && m2[q].last == -1 && m2[q].min == 0.0
		      && m2[q].max == 0.0, "... in the value: 0");

	/* signed zeros and infinities: -0.0 < +0.0, +-Inf win, in u of line (j, i) = (1, 2) along z */
	{
		const long W = N1 + 2*B, row = W*(N2 + 2*B);
		const double planted[N3] = { 0.0, -0.0, -INFINITY, INFINITY };
		for(k=0;k<N3;k++) x[(k+B)*row + (1+B)*W + 2 + B] = planted[k];
		CHECK(pft_map_host(&g, x, &pu, NULL, 0, m0) == 0, "planted");
		CHECK(m0[1*N1 + 2].min == -INFINITY && m0[1*N1 + 2].max == INFINITY && m0[1*N1 + 2].nonfinite == 2
		      && m0[1*N1 + 2].nonzero == 2 && m0[1*N1 + 2].first == 2 && m0[1*N1 + 2].last == 3, "+-Inf win");
		x[(2+B)*row + (1+B)*W + 2 + B] = NAN; x[(3+B)*row + (1+B)*W + 2 + B] = NAN;
		CHECK(pft_map_host(&g, x, &pu, NULL, 0, m0) == 0, "planted zeros");
		CHECK(m0[1*N1 + 2].min == 0.0 && signbit(m0[1*N1 + 2].min) && m0[1*N1 + 2].max == 0.0 && !signbit(m0[1*N1 + 2].max),
		      "-0.0 < +0.0");
		free(x);
		x = state(N3, 0, &S);
	}

	/* the combine laws on real records */
	CHECK(pft_map_host(&g, x, &pu, &pp, 1, m1) == 0, "records");
	{
		pft_map_px a = m1[2*N1], b = m1[3*N1 + 1], c = m1[0], ab, ba, l, r;
		ab = a; pft_map_combine(1, &ab, &b);
		ba = b; pft_map_combine(1, &ba, &a);
		CHECK(memcmp(&ab, &ba, sizeof ab) == 0 && ab.selected == a.selected + b.selected, "commutative");
		l = ab; pft_map_combine(1, &l, &c);
		r = b; pft_map_combine(1, &r, &c);
		t = a; pft_map_combine(1, &t, &r);
		CHECK(memcmp(&l, &t, sizeof l) == 0, "associative");
		l = a; pft_map_combine(1, &l, &neutral);
		r = neutral; pft_map_combine(1, &r, &a);
		CHECK(memcmp(&l, &a, sizeof l) == 0 && memcmp(&r, &a, sizeof r) == 0, "the neutral record is neutral");
		CHECK(pft_map_combine(1, NULL, &a) == -2 && pft_map_combine(1, &l, NULL) == -2 && pft_map_combine(-1, &l, &a) == -2
		      && pft_map_combine(0, &l, &a) == 0, "combine refuses");
	}

	/* slabs of 2 + 1 + 1 planes against one slab: axis 0 combines, axes 1 and 2 put rows together */
	for(axis=0;axis<3;axis++) {
		static const int n3s[3] = { 2, 1, 1 }, firsts[3] = { 0, 2, 3 };
		pft_map_px whole[N3*N1], parts[N3*N1], piece[N3*N1];
		int s, n;
		CHECK(pft_map_host(&g, x, &pu, &pp, axis, whole) == 0 && pft_map_dims(&g, axis, &rows, &cols) == 0, "one slab");
		n = rows * cols;
		for(q=0;q<n;q++) pft_map_init(&parts[q]);
		for(s=2;s>=0;s--) {          /* (in another order than the planes') */
			pft_grid gs;
			long Ss;
			double * xs = state(n3s[s], firsts[s], &Ss);
			int rs, cs;
			grid(&gs, n3s[s], firsts[s]);
			CHECK(pft_map_host(&gs, xs, &pu, &pp, axis, piece) == 0 && pft_map_dims(&gs, axis, &rs, &cs) == 0, "a slab");
			if(axis == 0) pft_map_combine(n, parts, piece);
			else memcpy(parts + firsts[s]*cols, piece, sizeof(pft_map_px)*(size_t)(rs*cs));
			free(xs);
		}
		CHECK(memcmp(parts, whole, sizeof(pft_map_px)*(size_t)n) == 0, "slabs == one slab");
	}

	/* every refusal; no refused call writes */
	{
		const int bad_op[1] = { 2 }, in_op[1] = { 101 };
		const double in_arg[1] = { 9 };
		const pft_hist_prog pbad = { 1, bad_op, u_arg }, pin = { 1, in_op, in_arg }, pnone = { 0, u_op, u_arg },
		                    pnull = { 1, NULL, u_arg }, plong = { PFT_FORMULA_MAX_ENTRIES + 1, u_op, u_arg };
		pft_grid none = g, huge = g;
		none.n3 = 0;
		huge.n1 = 2048; huge.n2 = 1024; huge.n3 = 1024;
		m0[0].selected = -77;
		CHECK(pft_map_host(NULL, x, &pu, NULL, 0, m0) == -2 && pft_map_host(&g, NULL, &pu, NULL, 0, m0) == -2
		      && pft_map_host(&g, x, NULL, NULL, 0, m0) == -2 && pft_map_host(&g, x, &pu, NULL, 0, NULL) == -2, "NULL arguments");
		CHECK(pft_map_host(&g, x, &pbad, NULL, 0, m0) == -2 && pft_map_host(&g, x, &pu, &pbad, 0, m0) == -2
		      && pft_map_host(&g, x, &pin, NULL, 0, m0) == -2 && pft_map_host(&g, x, &pnone, NULL, 0, m0) == -2
		      && pft_map_host(&g, x, &pnull, NULL, 0, m0) == -2 && pft_map_host(&g, x, &plong, NULL, 0, m0) == -2, "bad programs");
		CHECK(pft_map_host(&g, x, &pu, NULL, -1, m0) == -2 && pft_map_host(&g, x, &pu, NULL, 3, m0) == -2, "a bad axis");
		CHECK(pft_map_host(&none, x, &pu, NULL, 0, m0) == -2 && pft_map_host(&huge, x, &pu, NULL, 0, m0) == -2,
		      "a grid without cells, with 2^31");
		CHECK(pft_map_dims(NULL, 0, &rows, &cols) == -2 && pft_map_dims(&g, 3, &rows, &cols) == -2
		      && pft_map_dims(&g, 0, NULL, &cols) == -2 && pft_map_dims(&none, 0, &rows, &cols) == -2, "dims refuses");
		CHECK(m0[0].selected == -77, "no refused call writes");
	}

	/* 1 thread against 4, word for word */
	for(axis=0;axis<3;axis++) {
		omp_set_num_threads(4);
		CHECK(pft_map_host(&g, x, &pu, &pp, axis, m1) == 0 && pft_map_dims(&g, axis, &rows, &cols) == 0, "4 threads");
		omp_set_num_threads(1);
		CHECK(pft_map_host(&g, x, &pu, &pp, axis, again) == 0, "1 thread");
		CHECK(memcmp(m1, again, sizeof(pft_map_px)*(size_t)(rows*cols)) == 0, "1 thread == 4 threads");
	}

	free(x);
	if(failures) { printf("pft_map_selftest: %d failure(s)\n", failures); return 1; }
	printf("pft_map_selftest: ok\n");
	return 0;
}
