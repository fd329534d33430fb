/*
 * pft_ic_nodes.h -- host-internal: the node loop of intertrack.c:1950-1991 that pft_ic_eval (f1) and
 * pft_formula_host (f12) share, and the entries of pft_frontend.c the latter needs.
 */
#ifndef PFT_IC_NODES_H
#define PFT_IC_NODES_H

#include "../../include/pft_frontend.h"

/* called at every interior node of a plane: idx its index within one field of the padded host
   array, in[0..5] its x, y, z, _x, _y, _z (in[6..8] are the caller's) */
typedef void (*pft_ic_node_fn)(void * ctx, long idx, double * in);

/* the interior nodes of plane k of this slab in the reference's order (j, then i), with the node
   coordinates formed as intertrack.c:1958-1971 */
static inline void pft_ic_plane_nodes(const pft_grid * g, int k, pft_ic_node_fn fn, void * ctx)
{
	const long N1 = g->n1 + 2*PFT_BCOND_THICKNESS, N2 = g->n2 + 2*PFT_BCOND_THICKNESS;
	double in[9];
	int j, ii;
	const double _z = (0.5 + k + g->first_row) / g->total_n3;    /* intertrack.c:1958-1960 */
	in[5] = _z; in[2] = g->L3 * _z;
	in[6] = in[7] = in[8] = 0.0;
	for(j = 0; j < g->n2; j++) {
		const double _y = (0.5 + j) / g->n2;
		in[4] = _y; in[1] = g->L2 * _y;
		for(ii = 0; ii < g->n1; ii++) {
			const long idx = (k + PFT_BCOND_THICKNESS)*N1*N2 + (j + PFT_BCOND_THICKNESS)*N1 + ii + PFT_BCOND_THICKNESS;
			const double _x = (0.5 + ii) / g->n1;
			in[3] = _x; in[0] = g->L1 * _x;
			fn(ctx, idx, in);
		}
	}
}

/* pft_frontend.c: 0 for a valid program (known operators, inputs 0..8, a stack that never
   underflows, stays within the host's and ends at one value), else -2 */
int pft_ic_validate(int n, const int * op, const double * arg);
/* pft_frontend.c: the program on the inputs in[9] with the host's full operator set; *err = 1 when
   a math error ended the evaluation (the result is then 0) */
double pft_ic_run_host(int n, const int * op, const double * arg, const double * in, int * err);

#endif
