/*
 * pft_formula.h -- f12: formula diagnostics.  Any expression of the parameter file's language over
 * the node inputs x, y, z, _x, _y, _z, u, p, gl (and whatever constants the case defines) is
 * evaluated at every interior cell of a state and reduced exactly: what scripts/avg.sh and
 * scripts/freezing_point_depression.sh get from a snapshot with their FORMULA= line, ncap2 and ncwa
 * (the average, or -y mabs), without the download and without a summation order.  pft_diag (f5) and
 * pft_means (f6) are special cases: `p>0.5` counts the ice, `u` sums the temperature.
 *
 * A formula arrives as the postfix program of frontend.Evaluator.compile (pft_frontend.h: the
 * operator codes, inputs 0..8).  A math error at a cell (division by zero, sqrt of a negative,
 * ...) yields the value 0 there, as the reference's Eval() and the IC path.
 *
 * Every number of a record is an integer or comes from integer comparisons: counts, ordered keys
 * for the extrema, the exact accumulator pft_xsum for the sum.  So a record is the same bits for
 * every thread count, grid of workgroups, arrival order and Z-decomposition.
 *
 * Conventions as pft_means.h: extern "C"; every call returns int (0 = OK, -2 = bad arguments).
 * The device twin of pft_formula_host is pft_slab_formulas (below), the solver-level collective
 * pft_solver_formulas (pft_solver.h).
 */
#ifndef PFT_FORMULA_H
#define PFT_FORMULA_H

#include "pft_frontend.h"
#include "pft_means.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PFT_FORMULA_MAX 8             /* programs per call */
#define PFT_FORMULA_MAX_ENTRIES 256   /* program entries per call, all programs together */

typedef struct {
	long long cells;      /* interior cells evaluated */
	long long n;          /* cells whose value is finite: they entered sum */
	long long nonzero;    /* value != 0 -- the language's "true" (so a NaN counts) */
	long long nonfinite;  /* value NaN or +-Inf; cells == n + nonfinite */
	double min, max;      /* over values that are not NaN; +Inf / -Inf when none; -0.0 < +0.0 (pft_diag's rule) */
	double maxabs;        /* max |v| over values that are not NaN, 0.0 when none; +-Inf wins, a NaN never */
	pft_xsum sum;         /* exact, pft_means.h's rule: +-0 adds nothing, non-finite left out */
} pft_fdiag;

/* the record of no cells: zero counts and words, min = +Inf, max = -Inf, maxabs = 0.0 -- the
   neutral element of pft_fdiag_combine (a zeroed struct is NOT: its min and max are 0.0) */
void pft_fdiag_init(pft_fdiag * d);

/* into = the record of both sets of cells: counts and words add, min / max / maxabs by the
   ordered keys.  Associative and commutative bit for bit.  0, or -2 (NULL). */
int pft_fdiag_combine(pft_fdiag * into, const pft_fdiag * other);

/* The records of nprog programs (program f: lens[f] entries, concatenated in ops / args) over the
   interior of a host array in the reference's padded layout.  Each program runs at every interior
   node with the node inputs of pft_ic_eval (x = L1*_x, _x = (0.5+i)/n1; z with g->first_row and
   g->total_n3; u, p, gl read from x_host_padded, which is not written) and the host's full
   operator set with the C library: every valid program is accepted.  total[f]: program f's
   record; per_plane (optional, g->n3 * nprog records): entry f*g->n3 + k is program f's record of
   this slab's plane k (global row g->first_row + k); total[f] is their combination.  OpenMP over
   the planes; integer sums, so the thread count does not matter.
   0; -2: NULL, a bad program, nprog outside 1..PFT_FORMULA_MAX, more than PFT_FORMULA_MAX_ENTRIES
   entries, a grid without cells or with more than 2^31 - 1. */
int pft_formula_host(const pft_grid * g, const double * x_host_padded, int nprog, const int * lens,
                     const int * ops, const double * args, pft_fdiag * total, pft_fdiag * per_plane);

/* One program compiled for the device against the slab's grid: pft_ic_compile (constants folded,
   one-coordinate subexpressions as per-axis tables, z tables for this slab's planes) with one more
   rule.  The operators C and P loop as often as their operand says; on the device such a loop
   would run as long as a cell's value asks, so here they are device-eligible only inside the
   subexpressions the host folds.  A C or P left in the residual program makes the formula "not
   device-exact".  0: compiled (free it with pft_ic_prog_free); 1: not device-exact (pow or a libm
   function, C or P over a field or several coordinates, a stack deeper than the device's): use
   pft_formula_host; -2 a bad program; -1 out of memory.  What the IC path accepts
   (pft_ic_compile) does not change. */
int pft_formula_compile(const pft_grid * g, int n, const int * op, const double * arg, pft_ic_prog * out);

/* The device twin: the records of nprog compiled programs (pft_formula_compile for this slab's
   grid) over interior planes 1..n3 of buffer `buf` -- the words and counts of pft_formula_host of
   the same state.  Two kernels on the compute stream.  The first has one workgroup column per
   program (blockIdx.y); a workgroup's work items are segments of one interior plane, read with
   16-byte loads like the means kernel (a field the program never pushes is not loaded; ghost and
   far planes are never read).  Every cell's value comes from the operators of csrc/pft_ic_ops.h
   with the evaluation stack in LDS.  Counts go by ballot and popcount, extrema through ordered
   keys and 64-bit integer atomic max, the sum through the means kernel's digit accumulation into a
   record per plane; the second kernel combines the planes' records.  No floating-point add and no
   compare-and-swap.  The accumulators are zeroed on the stream by every call; results arrive
   through pinned host memory under the slab's bounded wait; a poisoned slab refuses as
   pft_slab_means.  total: nprog records; per_plane: optional, n3 * nprog records as above.
   PFT_DIAG_WGS caps the workgroups per program here too.
   0; 1: a program is not device-exact (an operator outside pft_ic_op_device, a C or P, a stack
   deeper than PFT_IC_STACK -- what pft_formula_compile answers with 1): nothing is launched; -2: bad
   arguments, a bad program (an unknown operator, a stack that underflows or does not end at one
   value, tables of another grid), limits exceeded, more than 2^31 - 1 cells: nothing is launched
   either. */
int pft_slab_formulas(pft_slab * s, int buf, int nprog, const pft_ic_prog * progs, pft_fdiag * total,
                      pft_fdiag * per_plane);
/* HIP-event timing of that kernel pair (scripts/formula_time.py), as pft_slab_means_timing */
int pft_slab_formulas_timing(pft_slab * s, int on);
int pft_slab_formulas_last_ms(pft_slab * s, double * ms);

#ifdef __cplusplus
}
#endif
#endif
