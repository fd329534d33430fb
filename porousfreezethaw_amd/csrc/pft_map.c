/*
 * pft_map.c -- f15: the map record, its combine rule and its host twin (include/pft_map.h).
 * pft_map_host is the host-layout twin of the device map (map_kernel, pft_reduce.hip), which must
 * give the same records.
 *
 * Host C99, OpenMP over the planes like pft_hist_host.  Every number is a count, an index or an
 * extremum under an integer key, so the threads' records merge to the same bits in any order.
 */
#include "../../include/pft_map.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "pft_ic_nodes.h"

/* the total order of the non-NaN doubles, -0.0 < +0.0 (pft_formula.c's fkey, diag_key on the device) */
static uint64_t mkey(double x)
{
	uint64_t b;
	memcpy(&b, &x, 8);
	return (b >> 63) ? ~b : (b | (1ULL << 63));
}

void pft_map_init(pft_map_px * px)
{
	if(!px) return;
	memset(px, 0, sizeof *px);
	px->min = INFINITY;
	px->max = -INFINITY;
	px->first = px->last = -1;
}

int pft_map_combine(long n, pft_map_px * into, const pft_map_px * other)
{
	long q;
	if(!into || !other || n < 0) return -2;
	for(q = 0; q < n; q++) {
		pft_map_px * a = &into[q];
		const pft_map_px * b = &other[q];
		a->selected += b->selected;
		a->nonzero += b->nonzero;
		a->nonfinite += b->nonfinite;
		/* (a NaN is in no record that these calls made; one from elsewhere never replaces a value) */
		if(b->min == b->min && (a->min != a->min || mkey(b->min) < mkey(a->min))) a->min = b->min;
		if(b->max == b->max && (a->max != a->max || mkey(b->max) > mkey(a->max))) a->max = b->max;
		if(b->first >= 0 && (a->first < 0 || b->first < a->first)) a->first = b->first;
		if(b->last > a->last) a->last = b->last;
	}
	return 0;
}

static int grid_ok(const pft_grid * g)
{
	return g && g->n1 >= 1 && g->n2 >= 1 && g->n3 >= 1 && (long long)g->n1 * g->n2 * g->n3 <= 0x7fffffffLL;
}

int pft_map_dims(const pft_grid * g, int axis, int * rows, int * cols)
{
	if(!grid_ok(g) || !rows || !cols || axis < 0 || axis > 2) return -2;
	*rows = axis == 0 ? g->n2 : g->n3;
	*cols = axis == 2 ? g->n2 : g->n1;
	return 0;
}

typedef struct {
	const pft_hist_prog * value, * mask;
	const double * x;
	long S;
	int axis, n1, k, first_row;
	long node;              /* nodes of this plane seen so far: j * n1 + i */
	pft_map_px * map;       /* axis 0: the thread's partial map; axes 1, 2: the slab's */
} mhost_ctx;

static void mhost_node(void * ctx, long idx, double * in)
{
	mhost_ctx * c = (mhost_ctx *)ctx;
	const int j = (int)(c->node / c->n1), i = (int)(c->node - (long)j * c->n1);
	pft_map_px * px;
	long long at;
	double v;
	int e;
	c->node++;
	in[6] = c->x[idx]; in[7] = c->x[c->S + idx]; in[8] = c->x[2*c->S + idx];
	/* (a math error yields 0: not selected; a NaN is "true") */
	if(c->mask && !(pft_ic_run_host(c->mask->n, c->mask->op, c->mask->arg, in, &e) != 0)) return;
	v = pft_ic_run_host(c->value->n, c->value->op, c->value->arg, in, &e);
	if(c->axis == 0) { px = &c->map[c->node - 1]; at = (long long)c->first_row + c->k; }
	else if(c->axis == 1) { px = &c->map[(long)c->k * c->n1 + i]; at = j; }
	else { px = &c->map[j]; at = i; }                    /* (map: the plane's row of n2 pixels) */
	px->selected++;
	if(v != 0) {
		px->nonzero++;
		if(px->first < 0 || at < px->first) px->first = at;
		if(at > px->last) px->last = at;
	}
	if(!(fabs(v) < INFINITY)) px->nonfinite++;
	if(v == v) {
		if(mkey(v) < mkey(px->min)) px->min = v;
		if(mkey(v) > mkey(px->max)) px->max = v;
	}
}

static int mprog_ok(const pft_hist_prog * p)
{
	return p && p->n >= 1 && p->n <= PFT_FORMULA_MAX_ENTRIES && p->op && p->arg && !pft_ic_validate(p->n, p->op, p->arg);
}

int pft_map_host(const pft_grid * g, const double * x, const pft_hist_prog * value, const pft_hist_prog * mask,
                 int axis, pft_map_px * out)
{
	const int B = PFT_BCOND_THICKNESS;
	int k, rows, cols, failed = 0;
	long S, q, n;
	if(!x || !out || pft_map_dims(g, axis, &rows, &cols)) return -2;
	if(!mprog_ok(value) || (mask && !mprog_ok(mask))) return -2;
	S = (long)(g->n1 + 2*B) * (g->n2 + 2*B) * (g->n3 + 2*B);
	n = (long)rows * cols;
	for(q = 0; q < n; q++) pft_map_init(&out[q]);
	#pragma omp parallel
	{
		/* axis 0: every plane meets every pixel, so a thread gathers its planes in a map of its own;
		   axes 1 and 2: plane k has rows of its own in `out` */
		pft_map_px * mine = axis == 0 ? (pft_map_px *)malloc(sizeof(pft_map_px) * (size_t)n) : out;
		mhost_ctx c;
		long w;
		c.value = value; c.mask = mask; c.x = x; c.S = S; c.axis = axis; c.n1 = g->n1; c.first_row = g->first_row;
		c.map = mine;
		if(!mine) {
			#pragma omp atomic write
			failed = 1;
		} else if(axis == 0) {
			for(w = 0; w < n; w++) pft_map_init(&mine[w]);
		}
		#pragma omp for schedule(static) nowait
		for(k = 0; k < g->n3; k++) {
			if(!mine) continue;
			c.k = k;
			c.node = 0;
			c.map = axis == 2 ? out + (long)k * g->n2 : mine;
			pft_ic_plane_nodes(g, k, mhost_node, &c);
		}
		if(axis == 0 && mine) {
			#pragma omp critical(pft_map_merge)
			pft_map_combine(n, out, mine);
			free(mine);
		}
	}
	return failed ? -1 : 0;
}
