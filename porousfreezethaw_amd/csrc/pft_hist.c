/*
 * pft_hist.c -- f13: the histogram record, its rule and its host twin (include/pft_hist.h).
 * pft_hist_host is the host-layout twin of the device histogram (hist_kernel, pft_reduce.hip), which
 * must give the same counts.
 *
 * Host C99, OpenMP over the planes like pft_formula_host.  Every number is an integer count, so the
 * threads' records merge to the same bits in any order.
 */
#include "../../include/pft_hist.h"

#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "pft_ic_nodes.h"

int pft_hist_check(int nbins, const double * edges)
{
	int i;
	if(nbins < 1 || nbins > PFT_HIST_MAX_BINS || !edges) return -2;
	for(i = 0; i <= nbins; i++) {
		if(!(fabs(edges[i]) < INFINITY)) return -2;                /* NaN, +-Inf */
		if(i > 0 && !(edges[i - 1] < edges[i])) return -2;         /* (-0.0 < +0.0 is false) */
	}
	return 0;
}

int pft_hist_bin(int nbins, const double * edges, double v)
{
	int lo = 0, hi = nbins + 1;      /* the number of edges <= v lies in [lo, hi] */
	if(v != v) return PFT_HIST_NAN;
	if(v < edges[0]) return PFT_HIST_UNDER;
	if(v > edges[nbins]) return PFT_HIST_OVER;
	while(lo < hi) {
		const int mid = (lo + hi + 1) / 2;                        /* 1 .. nbins + 1 */
		if(edges[mid - 1] <= v) lo = mid;
		else hi = mid - 1;
	}
	return lo > nbins ? nbins - 1 : lo - 1;                        /* v == edges[nbins]: the last bin */
}

int pft_hist_combine(int nbins, pft_hist_head * into, long long * into_counts, const pft_hist_head * other,
                     const long long * other_counts)
{
	int b;
	if(!into || !into_counts || !other || !other_counts || nbins < 1 || nbins > PFT_HIST_MAX_BINS) return -2;
	into->cells += other->cells;
	into->selected += other->selected;
	into->nan += other->nan;
	into->under += other->under;
	into->over += other->over;
	for(b = 0; b < nbins; b++) into_counts[b] += other_counts[b];
	return 0;
}

typedef struct {
	const pft_hist_prog * value, * mask;
	const double * x, * edges;
	long S;
	int nbins;
	pft_hist_head * head;   /* the plane's record */
	long long * counts;
} hhost_ctx;

static void hhost_node(void * ctx, long idx, double * in)
{
	const hhost_ctx * c = (const hhost_ctx *)ctx;
	int e, b;
	in[6] = c->x[idx]; in[7] = c->x[c->S + idx]; in[8] = c->x[2*c->S + idx];
	c->head->cells++;
	/* (a math error yields 0: not selected; a NaN is "true") */
	if(c->mask && !(pft_ic_run_host(c->mask->n, c->mask->op, c->mask->arg, in, &e) != 0)) return;
	c->head->selected++;
	b = pft_hist_bin(c->nbins, c->edges, pft_ic_run_host(c->value->n, c->value->op, c->value->arg, in, &e));
	if(b == PFT_HIST_NAN) c->head->nan++;
	else if(b == PFT_HIST_UNDER) c->head->under++;
	else if(b == PFT_HIST_OVER) c->head->over++;
	else c->counts[b]++;
}

static int hprog_ok(const pft_hist_prog * p)
{
	return p && p->n >= 1 && p->n <= PFT_FORMULA_MAX_ENTRIES && p->op && p->arg && !pft_ic_validate(p->n, p->op, p->arg);
}

int pft_hist_host(const pft_grid * g, const double * x, const pft_hist_prog * value, const pft_hist_prog * mask,
                  int nbins, const double * edges, pft_hist_head * total, long long * counts,
                  pft_hist_head * plane_heads, long long * plane_counts)
{
	const int B = PFT_BCOND_THICKNESS;
	int k, failed = 0;
	long S;
	if(!g || !x || !total || !counts || g->n1 < 1 || g->n2 < 1 || g->n3 < 1) return -2;
	if((long long)g->n1 * g->n2 * g->n3 > 0x7fffffffLL) return -2;
	if(pft_hist_check(nbins, edges) || !hprog_ok(value) || (mask && !hprog_ok(mask))) return -2;
	S = (long)(g->n1 + 2*B) * (g->n2 + 2*B) * (g->n3 + 2*B);
	memset(total, 0, sizeof *total);
	memset(counts, 0, sizeof(long long) * (size_t)nbins);
	#pragma omp parallel
	{
		/* t: this thread's planes together; m: the plane at hand */
		pft_hist_head th, mh;
		long long * tc = (long long *)calloc(2 * (size_t)nbins, sizeof(long long));
		long long * mc = tc ? tc + nbins : NULL;
		hhost_ctx c;
		memset(&th, 0, sizeof th);
		c.value = value; c.mask = mask; c.x = x; c.edges = edges; c.S = S; c.nbins = nbins; c.head = &mh; c.counts = mc;
		if(!tc) {
			#pragma omp atomic write
			failed = 1;
		}
		#pragma omp for schedule(static) nowait
		for(k = 0; k < g->n3; k++) {
			if(!tc) continue;
			memset(&mh, 0, sizeof mh);
			memset(mc, 0, sizeof(long long) * (size_t)nbins);
			pft_ic_plane_nodes(g, k, hhost_node, &c);
			if(plane_heads) plane_heads[k] = mh;
			if(plane_counts) memcpy(plane_counts + (size_t)k * nbins, mc, sizeof(long long) * (size_t)nbins);
			pft_hist_combine(nbins, &th, tc, &mh, mc);
		}
		if(tc) {
			#pragma omp critical(pft_hist_merge)
			pft_hist_combine(nbins, total, counts, &th, tc);
		}
		free(tc);
	}
	return failed ? -1 : 0;
}
