/*
 * pft_hist.h -- f13: histograms of formula values.  The value of a formula of the parameter file's
 * language (pft_formula.h: the postfix program of frontend.Evaluator.compile over the node inputs)
 * at every interior cell that an optional second formula, the mask, selects, counted into bins with
 * explicit edges: what numpy.histogram(values[selected], bins=edges) gives of a downloaded state,
 * without the download.  pft_formula.h answers "how much"; this answers "how is it distributed".
 *
 * Selection: a cell is selected when there is no mask, or when the mask's value is != 0 -- the
 * language's "true", so a NaN selects, as pft_fdiag's nonzero counts it.  A math error in either
 * program yields 0 at that cell, as the reference's Eval(): for the mask the cell is not selected.
 *
 * Binning of a selected cell's value v, by IEEE comparisons only (pft_hist_bin is the rule):
 *   v != v                  -> nan
 *   v <  edges[0]           -> under   (-Inf goes here)
 *   v >  edges[nbins]       -> over    (+Inf goes here)
 *   otherwise bin b with edges[b] <= v < edges[b+1]; v == edges[nbins] belongs to the last bin;
 *   -0.0 compares as 0.0.
 * With NaN left out this is numpy.histogram with explicit edges.
 *
 * Every number of a record is an integer count, so a record is the same bits for every thread
 * count, grid of workgroups, arrival order and Z-decomposition.
 *
 * Conventions as pft_formula.h: extern "C"; every call returns int (0 = OK, -2 = bad arguments).
 * The device twin of pft_hist_host is pft_slab_hist (below), the solver-level collective
 * pft_solver_hist (pft_solver.h).
 */
#ifndef PFT_HIST_H
#define PFT_HIST_H

#include "pft_formula.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PFT_HIST_MAX_BINS 1024

/* a record is a head and `long long counts[nbins]`;
   invariant: selected == nan + under + over + the sum of counts */
typedef struct {
	long long cells;      /* interior cells evaluated */
	long long selected;   /* cells the mask selects (all of them without a mask) */
	long long nan;        /* selected cells whose value is NaN */
	long long under;      /* selected cells with value < edges[0] */
	long long over;       /* selected cells with value > edges[nbins] */
} pft_hist_head;

/* a formula as the host takes it: n entries of frontend.Evaluator.compile's postfix program */
typedef struct {
	int n;
	const int * op;
	const double * arg;
} pft_hist_prog;

/* The judge of a set of edges: 0 when nbins is in 1..PFT_HIST_MAX_BINS and the nbins + 1 edges are
   finite and strictly increasing as doubles compare; -2 otherwise (NULL, NaN, +-Inf, equal
   neighbours, a decreasing pair; -0.0 next to +0.0 compare equal and are refused). */
int pft_hist_check(int nbins, const double * edges);

/* The rule above for one value on checked edges: the bin 0..nbins-1, or PFT_HIST_UNDER,
   PFT_HIST_OVER, PFT_HIST_NAN. */
#define PFT_HIST_UNDER (-1)
#define PFT_HIST_OVER (-2)
#define PFT_HIST_NAN (-3)
int pft_hist_bin(int nbins, const double * edges, double v);

/* into = the record of both sets of cells: every count adds.  Associative and commutative; the
   zeroed record is the neutral element.  0, or -2 (NULL, nbins outside 1..PFT_HIST_MAX_BINS). */
int pft_hist_combine(int nbins, pft_hist_head * into, long long * into_counts, const pft_hist_head * other,
                     const long long * other_counts);

/* The histogram of `value` over the cells that `mask` (NULL: every cell) selects, over the interior
   of a host array in the reference's padded layout (not written): the node loop and the node inputs
   of pft_formula_host, the host's full operator set with the C library, so every valid program is
   accepted.  total / counts[nbins]: the slab's record; plane_heads (optional, g->n3 heads) and
   plane_counts (optional, g->n3 * nbins counts, row k for this slab's plane k, global row
   g->first_row + k): the planes' records, whose sum the slab's is.  OpenMP over the planes; integer
   sums, so the thread count does not matter.
   0; -2: NULL, a bad program, edges that pft_hist_check refuses, a grid without cells or with more
   than 2^31 - 1. */
int pft_hist_host(const pft_grid * g, const double * x_host_padded, const pft_hist_prog * value,
                  const pft_hist_prog * mask, int nbins, const double * edges, pft_hist_head * total,
                  long long * counts, pft_hist_head * plane_heads, long long * plane_counts);

/* The device twin: the same counts of interior planes 1..n3 of buffer `buf`, for programs compiled
   with pft_formula_compile against this slab's grid (mask_prog NULL: no mask).  Two kernels on the
   compute stream.  hist_kernel has formula_kernel's traversal (work items are segments of one
   interior plane, 16-byte loads, only the fields either program pushes are loaded, ghost and far
   planes are never read, PFT_DIAG_WGS caps the workgroups); a cell's mask and then its value come
   from the wave interpreter of pft_slab_formulas on the same LDS stack column; the bin from a
   branch-free binary search of the edges in LDS with a wave-uniform trip count.  Head counts go by
   ballot and popcount; bin counts into 32-bit LDS counters, equal bins of a wave aggregated first;
   at the end of an item the non-zero words are added to the plane's row in global memory with
   64-bit integer atomics.  hist_total_kernel adds the planes' rows into the slab's.  Integers only.
   The accumulators are zeroed on the stream by every call; results arrive through pinned host
   memory under the slab's bounded wait; a poisoned slab refuses as pft_slab_formulas.
   0; 1: a program is not device-exact (as pft_slab_formulas): nothing is launched; -2: bad
   arguments, a bad program, edges that pft_hist_check refuses, limits exceeded: nothing is
   launched either. */
int pft_slab_hist(pft_slab * s, int buf, const pft_ic_prog * value_prog, const pft_ic_prog * mask_prog,
                  int nbins, const double * edges, pft_hist_head * head, long long * counts,
                  pft_hist_head * plane_heads, long long * plane_counts);
/* HIP-event timing of that kernel pair (scripts/hist_time.py), as pft_slab_formulas_timing */
int pft_slab_hist_timing(pft_slab * s, int on);
int pft_slab_hist_last_ms(pft_slab * s, double * ms);

#ifdef __cplusplus
}
#endif
#endif
