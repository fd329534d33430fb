/*
 * pft_formula.c -- f12: the formula-diagnostics record, its host twin and the compile rule of the
 * device route (include/pft_formula.h).  pft_formula_host is the host-layout twin of the device
 * reduction (formula_kernel, pft_reduce.hip), which must give the same counts and raw words.
 *
 * Host C99, OpenMP over the planes like pft_means_host.  Every number is an integer sum or an
 * integer comparison, so the threads' records merge to the same bits in any order.
 */
#include "../../include/pft_formula.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pft_ic_nodes.h"

/* pft_reduce.hip's diag_key: orders every non-NaN double as the double orders, -0.0 below +0.0 */
static uint64_t fkey(double x)
{
	uint64_t b;
	memcpy(&b, &x, 8);
	return (b >> 63) ? ~b : (b | (1ULL << 63));
}

void pft_fdiag_init(pft_fdiag * d)
{
	if(!d) return;
	memset(d, 0, sizeof *d);
	d->min = INFINITY;
	d->max = -INFINITY;
}

/* one value into a record */
static void fdiag_add(pft_fdiag * d, double v)
{
	d->cells++;
	if(v != 0) d->nonzero++;                 /* (a NaN is "true") */
	if(pft_xsum_add(&d->sum, v)) d->nonfinite++;
	else d->n++;
	if(v == v) {
		const double a = fabs(v);
		if(fkey(v) < fkey(d->min)) d->min = v;
		if(fkey(v) > fkey(d->max)) d->max = v;
		if(a > d->maxabs) d->maxabs = a;
	}
}

int pft_fdiag_combine(pft_fdiag * into, const pft_fdiag * other)
{
	if(!into || !other) return -2;
	into->cells += other->cells;
	into->n += other->n;
	into->nonzero += other->nonzero;
	into->nonfinite += other->nonfinite;
	/* (a NaN is in no record that these calls made; one from elsewhere never replaces a value) */
	if(other->min == other->min && (into->min != into->min || fkey(other->min) < fkey(into->min))) into->min = other->min;
	if(other->max == other->max && (into->max != into->max || fkey(other->max) > fkey(into->max))) into->max = other->max;
	if(other->maxabs > into->maxabs || into->maxabs != into->maxabs) into->maxabs = other->maxabs;
	pft_xsum_combine(&into->sum, &other->sum);
	return 0;
}

typedef struct {
	int nprog;
	const int * lens, * ops;
	const double * args, * x;
	long S;
	pft_fdiag * rec;       /* nprog records: the plane's */
} fhost_ctx;

static void fhost_node(void * ctx, long idx, double * in)
{
	const fhost_ctx * c = (const fhost_ctx *)ctx;
	int f, off = 0, e;
	in[6] = c->x[idx]; in[7] = c->x[c->S + idx]; in[8] = c->x[2*c->S + idx];
	for(f = 0; f < c->nprog; f++) {
		fdiag_add(&c->rec[f], pft_ic_run_host(c->lens[f], c->ops + off, c->args + off, in, &e));
		off += c->lens[f];
	}
}

/* the limits host and device share: 1..PFT_FORMULA_MAX programs, PFT_FORMULA_MAX_ENTRIES entries */
static int formula_limits(int nprog, const int * lens)
{
	int f, all = 0;
	if(nprog < 1 || nprog > PFT_FORMULA_MAX || !lens) return -2;
	for(f = 0; f < nprog; f++) {
		if(lens[f] < 1 || lens[f] > PFT_FORMULA_MAX_ENTRIES) return -2;
		all += lens[f];
	}
	return all > PFT_FORMULA_MAX_ENTRIES ? -2 : 0;
}

int pft_formula_host(const pft_grid * g, const double * x, int nprog, const int * lens, const int * ops,
                     const double * args, pft_fdiag * total, pft_fdiag * per_plane)
{
	const int B = PFT_BCOND_THICKNESS;
	int f, k, off = 0;
	long S;
	if(!g || !x || !ops || !args || !total || g->n1 < 1 || g->n2 < 1 || g->n3 < 1) return -2;
	if((long long)g->n1 * g->n2 * g->n3 > 0x7fffffffLL) return -2;
	if(formula_limits(nprog, lens)) return -2;
	for(f = 0; f < nprog; f++) {
		if(pft_ic_validate(lens[f], ops + off, args + off)) return -2;
		off += lens[f];
	}
	S = (long)(g->n1 + 2*B) * (g->n2 + 2*B) * (g->n3 + 2*B);
	for(f = 0; f < nprog; f++) pft_fdiag_init(&total[f]);
	#pragma omp parallel
	{
		pft_fdiag t[PFT_FORMULA_MAX], m[PFT_FORMULA_MAX];
		fhost_ctx c;
		int q;
		c.nprog = nprog; c.lens = lens; c.ops = ops; c.args = args; c.x = x; c.S = S; c.rec = m;
		for(q = 0; q < nprog; q++) pft_fdiag_init(&t[q]);
		#pragma omp for schedule(static) nowait
		for(k = 0; k < g->n3; k++) {
			for(q = 0; q < nprog; q++) pft_fdiag_init(&m[q]);
			pft_ic_plane_nodes(g, k, fhost_node, &c);
			for(q = 0; q < nprog; q++) {
				if(per_plane) per_plane[(size_t)q * g->n3 + k] = m[q];
				pft_fdiag_combine(&t[q], &m[q]);
			}
		}
		#pragma omp critical(pft_formula_merge)
		for(q = 0; q < nprog; q++) pft_fdiag_combine(&total[q], &t[q]);
	}
	return 0;
}

int pft_formula_compile(const pft_grid * g, int n, const int * op, const double * arg, pft_ic_prog * out)
{
	int rc, i;
	if(n > PFT_FORMULA_MAX_ENTRIES) return -2;
	rc = pft_ic_compile(g, n, op, arg, out);
	if(rc) return rc;
	/* C, P: a loop whose trip count is the operand.  Folded on the host they are gone from the
	   residual program; one that is left would loop on the device as long as a cell's value says */
	for(i = 0; i < out->n; i++)
		if(out->op[i] == 5 || out->op[i] == 6) { pft_ic_prog_free(out); return 1; }
	return 0;
}
