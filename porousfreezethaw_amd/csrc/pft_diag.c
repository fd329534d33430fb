/*
 * pft_diag.c -- f5: the ice diagnostics on a host array (include/pft_diag.h): the host-layout twin
 * of the device reduction (diag_kernel, pft_reduce.hip) and a second statement of its semantics,
 * written with plain comparisons where the kernel orders doubles by an integer key.
 *
 * Host C99, OpenMP over the planes like pft_ic_eval.  Every quantity is a count or a maximum, so
 * the threads' records merge to the same bits in any order (pft_diag_combine).
 */
#include "../../include/pft_diag.h"

#include <math.h>
#include <stddef.h>

/* a ranks above b; of the two zeros +0.0 ranks above -0.0 (the kernel's key order).  False when
   either is a NaN. */
static int above(double a, double b)
{
	return a > b || (a == b && signbit(b) && !signbit(a));
}

static void diag_clear(pft_diag * d)
{
	d->cells = d->ice = d->pore = d->ice_pore = d->nonfinite = 0;
	d->ice_u_maxabs = 0.0;
	d->u_min = d->p_min = INFINITY;
	d->u_max = d->p_max = -INFINITY;
}

int pft_diag_combine(pft_diag * into, const pft_diag * other)
{
	if(!into || !other) return -2;
	into->cells += other->cells;
	into->ice += other->ice;
	into->pore += other->pore;
	into->ice_pore += other->ice_pore;
	into->nonfinite += other->nonfinite;
	if(other->ice_u_maxabs > into->ice_u_maxabs) into->ice_u_maxabs = other->ice_u_maxabs;
	if(above(other->u_max, into->u_max)) into->u_max = other->u_max;
	if(above(into->u_min, other->u_min)) into->u_min = other->u_min;
	if(above(other->p_max, into->p_max)) into->p_max = other->p_max;
	if(above(into->p_min, other->p_min)) into->p_min = other->p_min;
	return 0;
}

int pft_diag_host(const pft_grid * g, const double * x, const pft_diag_opts * opts, pft_diag * out,
                  long long * ice_per_plane)
{
	const int B = PFT_BCOND_THICKNESS;
	double p_thr = 0.5, gl_thr = 0.5;
	long N1, row, S;
	int k;
	if(!g || !x || !out || g->n1 < 1 || g->n2 < 1 || g->n3 < 1) return -2;
	if(opts) { p_thr = opts->p_thr; gl_thr = opts->gl_thr; }
	N1 = g->n1 + 2L*B; row = N1*(g->n2 + 2L*B); S = row*(g->n3 + 2L*B);
	diag_clear(out);
	#pragma omp parallel
	{
		pft_diag d;
		diag_clear(&d);
		#pragma omp for schedule(static) nowait
		for(k=0;k<g->n3;k++) {
			long long plane_ice = 0;
			int j, i;
			for(j=0;j<g->n2;j++) {
				const double * u = x + PFT_VAR_U*S + (k+B)*row + (long)(j+B)*N1 + B;
				const double * p = u + (PFT_VAR_P - PFT_VAR_U)*S;
				const double * gl = u + (PFT_VAR_GL - PFT_VAR_U)*S;
				for(i=0;i<g->n1;i++) {
					const double uv = u[i], pv = p[i], gv = gl[i];
					const int ice = pv > p_thr, pore = gv < gl_thr;
					d.cells++;
					d.ice += ice;
					d.pore += pore;
					d.ice_pore += ice && pore;
					d.nonfinite += !(isfinite(uv) && isfinite(pv) && isfinite(gv));
					plane_ice += ice;
					if(ice && fabs(uv) > d.ice_u_maxabs) d.ice_u_maxabs = fabs(uv);   /* false on NaN */
					if(above(uv, d.u_max)) d.u_max = uv;
					if(above(d.u_min, uv)) d.u_min = uv;
					if(above(pv, d.p_max)) d.p_max = pv;
					if(above(d.p_min, pv)) d.p_min = pv;
				}
			}
			if(ice_per_plane) ice_per_plane[k] = plane_ice;
		}
		#pragma omp critical(pft_diag_merge)
		pft_diag_combine(out, &d);
	}
	return 0;
}
