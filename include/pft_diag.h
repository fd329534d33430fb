/*
 * pft_diag.h -- f5: the ice diagnostics of a state (u, p, gl), the quantities the reference
 * application publishes per snapshot: scripts/avg.sh averages (p > 0.5) over every NetCDF snapshot
 * with NCO (its commented alternative: gl < 0.5), scripts/freezing_point_depression.sh takes
 * ncwa -y mabs of (p > 0.5) * u.  Here they are counts and maxima over the interior cells: exact,
 * independent of the decomposition and of any order of evaluation -- no floating-point sum.
 *
 * Conventions: extern "C"; every call returns int (0 = OK, negative = error).  The device twin of
 * pft_diag_host is pft_slab_diag (pft_hip.h), the solver-level collective pft_solver_diag
 * (pft_solver.h).
 */
#ifndef PFT_DIAG_H
#define PFT_DIAG_H

#include "pft_model.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { double p_thr, gl_thr; } pft_diag_opts;     /* NULL = {0.5, 0.5}, the scripts' */

typedef struct {
	long long cells;        /* interior cells looked at */
	long long ice;          /* p  >  p_thr   (strict; a NaN is not ice)        avg.sh */
	long long pore;         /* gl <  gl_thr  (strict)                          avg.sh's commented formula */
	long long ice_pore;     /* both */
	long long nonfinite;    /* cells where u, p or gl is NaN or +-Inf */
	double ice_u_maxabs;    /* max |u| over ice cells, 0.0 when there is none: ncwa -y mabs of (p>0.5)*u;
	                           a NaN never wins (as in the error norm), +-Inf does */
	double u_min, u_max, p_min, p_max;   /* over cells whose value is not NaN; +Inf / -Inf when none.
	                                        Of -0.0 and +0.0 the max is +0.0 and the min -0.0 */
} pft_diag;

/* The diagnostics of the interior of a host array in the reference's padded layout (pft_model.h:
   per variable N1*N2*N3 doubles, ghost thickness 2); no ghost cell is read.  opts = NULL: the
   scripts' thresholds.  ice_per_plane (optional, g->n3 entries): the ice count of each interior
   plane of this slab, entry k for the global row g->first_row + k -- the freezing front.
   OpenMP over the planes; the result does not depend on the thread count.  0, or -2 (NULL or a
   grid without cells). */
int pft_diag_host(const pft_grid * g, const double * x_host_padded, const pft_diag_opts * opts,
                  pft_diag * out, long long * ice_per_plane);

/* into = into merged with other: counts add, maxima and minima are taken (a record of no cells is
   the neutral element: zero counts, ice_u_maxabs 0, u_min = p_min = +Inf, u_max = p_max = -Inf).
   Associative and commutative bit for bit.  0, or -2 (NULL). */
int pft_diag_combine(pft_diag * into, const pft_diag * other);

#ifdef __cplusplus
}
#endif
#endif
