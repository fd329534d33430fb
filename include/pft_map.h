/*
 * pft_map.h -- f15: 2-D maps of formula values.  The value of a formula of the parameter file's
 * language (pft_formula.h: the postfix program of frontend.Evaluator.compile over the node inputs)
 * at every interior cell that an optional second formula, the mask, selects, reduced along one axis
 * of the grid into one record per pixel of the other two: where the freezing front stands over each
 * (x, y), how thick the ice column is, the warmest ice along each line of sight -- without the
 * download.  pft_formula.h answers "how much", pft_hist.h "how is it distributed", this "where".
 *
 * axis numbers the axes of the interior array [k][j][i] as numpy does:
 *   axis 0 reduces z: the map is [n2][n1]
 *   axis 1 reduces y: the map is [n3][n1]   (a slab's own planes; [total_n3][n1] of the whole grid)
 *   axis 2 reduces x: the map is [n3][n2]   (                     [total_n3][n2]                  )
 *
 * Selection is pft_hist.h's rule word for word: a cell is selected when there is no mask, or when
 * the mask's value is != 0 -- the language's "true", so a NaN selects.  A math error in either
 * program yields 0 at that cell, as the reference's Eval(): for the mask the cell is not selected.
 *
 * Every number of a record is an integer count, an index, or the minimum / maximum of doubles under
 * pft_fdiag's order (-0.0 < +0.0, a NaN never wins, +-Inf does), so two partial maps combine
 * associatively and commutatively bit for bit, and a map is the same for every thread count, grid of
 * workgroups, chunking, arrival order and Z-decomposition.  There are no sums: an exact sum per pixel
 * would need pft_xsum's 66 words per pixel.  The mean of a 0/1 formula along a line is exact already:
 * nonzero / selected, one correctly rounded division.
 *
 * Conventions as pft_hist.h: extern "C"; every call returns int (0 = OK, -2 = bad arguments).
 * The device twin of pft_map_host is pft_slab_map (below), the solver-level collective
 * pft_solver_map (pft_solver.h).
 */
#ifndef PFT_MAP_H
#define PFT_MAP_H

#include "pft_hist.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one pixel: the selected cells of its line (56 bytes, no padding) */
typedef struct {
	long long selected;    /* selected cells */
	long long nonzero;     /* of them with value != 0 (the language's "true": a NaN counts) */
	long long nonfinite;   /* of them with a value that is NaN or +-Inf */
	double min, max;       /* over the selected values that are not NaN; +Inf / -Inf when there is none */
	long long first, last; /* the global index along the reduced axis of the first and of the last
	                          selected cell whose value is != 0; -1 when there is none */
} pft_map_px;

/* the neutral record (a zeroed struct is not: min, max, first, last) */
void pft_map_init(pft_map_px * px);

/* into[q] = the record of both sets of cells, for n pixels: counts add, min / max under pft_fdiag's
   order, first the smaller index, last the larger.  Associative and commutative; pft_map_init's
   record is the neutral element.  0, or -2 (NULL, n < 0). */
int pft_map_combine(long n, pft_map_px * into, const pft_map_px * other);

/* the shape of this slab's map: rows x cols = n2 x n1 (axis 0), n3 x n1 (axis 1), n3 x n2 (axis 2).
   0, or -2 (NULL, axis outside 0..2, a grid without cells or with more than 2^31 - 1). */
int pft_map_dims(const pft_grid * g, int axis, int * rows, int * cols);

/* The map of `value` over the cells that `mask` (NULL: every cell) selects, over the interior of a
   host array in the reference's padded layout (not written): the node loop and the node inputs of
   pft_formula_host, the host's full operator set with the C library, so every valid program is
   accepted.  out: rows * cols records (pft_map_dims), row-major.  For axis 0 it is this slab's
   partial map, with first / last as global z indices (g->first_row + k): the slabs' maps combine
   (pft_map_combine) to the whole grid's.  For axes 1 and 2 row k is this slab's plane k (global row
   g->first_row + k) and is complete.  OpenMP over the planes; integer merges, so the thread count
   does not matter.
   0; -2: NULL, a bad program, axis outside 0..2, a grid without cells or with more than 2^31 - 1. */
int pft_map_host(const pft_grid * g, const double * x_host_padded, const pft_hist_prog * value,
                 const pft_hist_prog * mask, int axis, pft_map_px * out);

/* The device twin: the same records of interior planes 1..n3 of buffer `buf`, for programs compiled
   with pft_formula_compile against this slab's grid (mask_prog NULL: no mask).  The slab does not
   know its place in the grid: for axis 0 first / last are the slab's own plane indices 0..n3-1
   (pft_solver_map adds the slab's first row).  One kernel on the compute stream, map_kernel<AXIS>,
   with the wave interpreter of pft_slab_formulas on the same LDS stack column, the mask and then the
   value as hist_kernel evaluates them.  Axes 0 and 1: a lane owns two neighbouring pixels and
   marches its chunk of the reduced axis with both pixels' accumulators in registers; axis 2:
   formula_kernel's traversal, a wave reducing each row its window touches by ballot and shuffle.
   Only the non-zero words go to the pixel's 7 accumulator words in global memory, with 64-bit
   integer atomicAdd / atomicMax; integers only.  Only the fields either program pushes are loaded,
   ghost and far planes are never read, PFT_DIAG_WGS caps the workgroups.  The accumulators are
   zeroed on the stream by every call; results arrive through pinned host memory under the slab's
   bounded wait; a poisoned slab refuses as pft_slab_hist.
   0; 1: a program is not device-exact (as pft_slab_formulas): nothing is launched; -2: bad
   arguments, a bad program, axis outside 0..2, limits exceeded: nothing is launched either. */
int pft_slab_map(pft_slab * s, int buf, const pft_ic_prog * value_prog, const pft_ic_prog * mask_prog, int axis,
                 pft_map_px * out_local);
/* HIP-event timing of that kernel (scripts/map_time.py), as pft_slab_hist_timing */
int pft_slab_map_timing(pft_slab * s, int on);
int pft_slab_map_last_ms(pft_slab * s, double * ms);

#ifdef __cplusplus
}
#endif
#endif
