/*
 * pft_solver.h -- libpft extensions around the reference solver ABI (RK_MPI_SAsolver.h).
 *
 * RK_MPI_SA_solve() keeps the reference contract: x is a host array, mirrored host->device at
 * entry and device->host at exit.  Drivers that keep the state on the GPU across calls (the
 * benchmark, long runs with rare snapshots) use pft_solve_ex() with the flags below; the loop,
 * its arithmetic and its control decisions are exactly those of RK_MPI_SA_solve().
 */
#ifndef PFT_SOLVER_H
#define PFT_SOLVER_H

#include "RK_MPI_SAsolver.h"
#include "pft_hip.h"
#include "pft_formula.h"
#include "pft_hist.h"
#include "pft_map.h"
#include "pft_io.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PFT_SOLVE_KEEP_DEVICE   1   /* leave x on the device at exit (no device->host copy) */
#define PFT_SOLVE_REUSE_DEVICE  2   /* the device already holds x from the previous call */

/* RK_MPI_SA_solve with an optional cap on attempted steps in this call (0 = none; returns 2
   when the cap stops the loop, with system->t and system->h set so that the next call
   continues the identical trajectory) and the flags above. */
int pft_solve_ex(FLOAT final_time, RK_MPI_S_SOLUTION * system, long max_steps_total, int flags);

/* copy the device-resident x back into system->x (host layout): after a pft_solve_ex call with
   PFT_SOLVE_KEEP_DEVICE, or from inside a Service_Callback on the fused path -- there the state
   lives on the device and system->x is only refreshed when solve returns, so a callback that
   reads x (a snapshot, say) downloads it first.  The reference's RKService (intertrack.c:1072-1116)
   reads only t and h. */
int pft_solver_download(RK_MPI_S_SOLUTION * system);

/* f5: the ice diagnostics (pft_diag.h; opts = NULL: thresholds 0.5) of the device-resident x of
   the fused path -- the published ice fraction is global->ice / global->cells -- without a
   download: one reduction kernel per slab (pft_slab_diag) and 96 bytes per rank.  Valid after any
   fused solve (RK_MPI_SA_solve or pft_solve_ex) and after a device IC.  global: the whole grid's
   record, the same bits on every rank; local (optional): this slab's; ice_per_plane (optional,
   this slab's n3 entries): the ice count of each of its planes, global rows first_row + k.
   Collective when the communicator has several ranks: the records are gathered
   (pft_comm_allgather) and merged in rank order, each with its rank's status, so every rank
   returns the same code.  From inside a Service_Callback it describes the state of the step just
   accepted, under the contract of pft_solver_download -- on one rank; with several ranks it
   refuses with -2 there (another rank's callback need not make the same call).
   0; -3: no initialised solver, or no resident state (before the first fused solve with a host IC;
   on the host-staged path) -- never stale numbers; -2: global is NULL, or see above;
   PFT_SOLVE_DEVICE_ERROR (below). */
int pft_solver_diag(const pft_diag_opts * opts, pft_diag * global, pft_diag * local, long long * ice_per_plane);

/* f6: the exact sums (pft_means.h) of the device-resident x, under the rules of pft_solver_diag:
   valid after any fused solve or device IC, -3 without a resident state (never stale numbers), 0
   from a Service_Callback on one rank and -2 there with several.  global: the whole grid's
   record, the same words on every rank; local (optional): this slab's; per_plane (optional, this
   slab's n3 records): one record per plane, global rows first_row + k.  Collective on several
   ranks: each rank reduces its slab (pft_slab_means) and its 2 144-byte record travels with its
   status by pft_comm_allgather_any (pft_comm.h: 9 rounds); the records are merged in rank order,
   every rank returns the same code. */
int pft_solver_means(const pft_diag_opts * opts, pft_means * global, pft_means * local, pft_means * per_plane);

/* f12: the formula diagnostics (pft_formula.h) of the device-resident x, under the rules of
   pft_solver_diag word for word: valid after any fused solve or device IC, -3 without an
   initialised solver or a resident state (never stale numbers), 0 from a Service_Callback on one
   rank and -2 there with several.  nprog programs (at most PFT_FORMULA_MAX, PFT_FORMULA_MAX_ENTRIES
   entries in all), program f with lens[f] entries, concatenated in ops / args (pft_frontend.h).
   Every rank compiles them first (pft_formula_compile) and the ranks agree the outcome before any
   device work: 1 when a program is not device-exact (nothing is launched: use pft_formula_host), -2
   for a bad program or limits exceeded, the same on every rank.  global: nprog records of the whole
   grid, the same bits on every rank; local (optional): this slab's; per_plane (optional, n3 * nprog
   records): entry f * n3 + k is program f's record of this slab's plane k.  Collective on several
   ranks: each rank reduces its slab (pft_slab_formulas) and its records travel with its status by
   pft_comm_allgather_any; they are merged in rank order and every rank returns the same code. */
int pft_solver_formulas(int nprog, const int * lens, const int * ops, const double * args, pft_fdiag * global,
                        pft_fdiag * local, pft_fdiag * per_plane);

/* f13: the histogram (pft_hist.h) of a formula's values over the cells a mask formula selects, of the
   device-resident x, under the rules of pft_solver_diag word for word: valid after any fused solve
   or device IC, -3 without an initialised solver or a resident state (never stale numbers), 0 from
   a Service_Callback on one rank and -2 there with several.  The value: nv entries in vops / vargs
   (pft_frontend.h); the mask: nm entries in mops / margs, or 0, NULL, NULL for none; nbins + 1
   edges (pft_hist_check).  Every rank checks and compiles first (pft_formula_compile) and the ranks
   agree the outcome before any device work: 1 when a program is not device-exact (nothing is
   launched: use pft_hist_host), -2 for a bad program, bad edges or limits exceeded, the same on
   every rank.  That first pft_comm_allgather round also carries a 64-bit hash of nbins, the edges
   and both programs: ranks that were given different histograms all return -2, before any device
   work.  global / global_counts[nbins]: the record of the whole grid, the same bits on every rank;
   local / local_counts (optional): this slab's; plane_heads (optional, n3 heads) and plane_counts
   (optional, n3 * nbins): this slab's planes'.  Collective on several ranks: each rank counts its
   slab (pft_slab_hist) and its record travels with its status by pft_comm_allgather_any (33 rounds
   for 1024 bins); the records are merged in rank order and every rank returns the same code. */
int pft_solver_hist(int nv, const int * vops, const double * vargs, int nm, const int * mops, const double * margs,
                    int nbins, const double * edges, pft_hist_head * global, long long * global_counts,
                    pft_hist_head * local, long long * local_counts, pft_hist_head * plane_heads,
                    long long * plane_counts);

/* f15: the map (pft_map.h) of a formula's values over the cells a mask formula selects, reduced along
   `axis` (0 z, 1 y, 2 x: numpy's numbering of the interior [k][j][i]), of the device-resident x,
   under the rules of pft_solver_hist word for word: valid after any fused solve or device IC, -3
   without an initialised solver or a resident state (never stale numbers), 0 from a
   Service_Callback on one rank and -2 there with several.  The value: nv entries in vops / vargs
   (pft_frontend.h); the mask: nm entries in mops / margs, or 0, NULL, NULL for none.  Every rank
   compiles first (pft_formula_compile) and the ranks agree the outcome before any device work: 1
   when a program is not device-exact (nothing is launched: use pft_map_host), -2 for a bad program,
   a bad axis or limits exceeded, the same on every rank.  That first pft_comm_allgather round also
   carries a 64-bit hash of the axis, of whether `global` is given and of both programs: ranks that
   were given different maps all return -2, before any device work.
   local (required): this slab's map, pft_map_dims records (pft_slab_map).  For axes 1 and 2 these
   are the slab's own rows first_row .. first_row + n3 - 1 of the whole grid's map, and complete;
   for axis 0 it is the slab's partial map, with first / last as global z indices.
   global (optional): the whole grid's map, the same bits on every rank: n2 x n1 records for axis 0
   (the ranks' partial maps combined in rank order), total_n3 x n1 or total_n3 x n2 for axes 1 and 2
   (the ranks' rows put together; every rank sends as many rows as the tallest slab has, the rest
   neutral).  It travels with the rank's status by pft_comm_allgather_any, 256 bytes per rank and
   round: a 200 x 200 map takes about 8 750 rounds (has the measured
   time); NULL skips it, and only the statuses travel.  A single rank makes no collective. */
int pft_solver_map(int nv, const int * vops, const double * vargs, int nm, const int * mops, const double * margs,
                   int axis, pft_map_px * global, pft_map_px * local);

/* f1 (after RK_MPI_SA_init): the default Params' initial condition (Params:9-21,
   intertrack.c:1880-2010) and, with with_beads, the glass beads (PrecalculateData,
   equation.c:459-530) computed on the device straight into the solver's state, bit for bit what
   pft_model_ic_default + PrecalculateData give on the host; system->x is not written (download it
   with pft_solver_download).  The next pft_solve_ex(..., PFT_SOLVE_REUSE_DEVICE) starts from it.
   Collective when the communicator has several ranks.  0, -3 (no RK_MPI_SA_init), -1 (beads
   requested but none set) or PFT_SOLVE_DEVICE_ERROR. */
int pft_solver_ic_default_device(int with_beads);
/* f1 for any icond formulas (intertrack.c:1831-2012): nprog compiled programs in the multi-pass
   order (frontend.py icond_programs), program p for field qs[p] with lens[p] entries, concatenated
   in ops/args (pft_frontend.h), then with with_beads the glass beads, all on the device into the
   solver's state -- bit for bit pft_ic_eval + PrecalculateData on the host.  Returns 1 without
   touching the device when a program is not device-exact (pft_ic_compile; every rank decides
   alike: evaluate on the host), else as pft_solver_ic_default_device; -2 a bad program. */
int pft_solver_ic_formulas_device(int nprog, const int * qs, const int * lens, const int * ops,
                                  const double * args, int with_beads);

/* f7: a snapshot dataset (pft_io.h) of the device-resident x, without a download.  It follows the
   validity rules of pft_solver_diag: -3 without an initialised solver or a resident state (never
   a stale file; nothing is created), -2 from a Service_Callback with several ranks.  Collective:
   rank 0 writes the header (pft_snapshot_create; the version of PFT_SNAP_VERSION(v) in flags, 0 =
   automatic), the ranks agree the status in an allreduce, which is also the barrier, every rank
   exports its slab's image (pft_slab_snapshot_export) and waits, bounded, until it is in pinned host
   memory; then the image goes to the background writer.  With PFT_SNAP_ASYNC the call returns
   there -- the image has left the device, so the next solve may overwrite x while the file is
   written -- otherwise it also waits for the write.  PFT_SNAP_DIRECT / PFT_SNAP_STAGED choose the
   host link of this call (default: staged, the faster one by a little -- 7.26 against 7.41 ms at
   200x200x400; env PFT_SNAP_LINK=0/1 = direct / staged for that A/B).  Every rank
   returns the same code: 0, a pft_io.h code (-1: I/O error) or PFT_SOLVE_DEVICE_ERROR.
   pft_solver_snapshot_wait (collective) returns once every rank's writes are done, with the agreed
   first error of the writes since the last wait. */
#define PFT_SNAP_ASYNC    1
#define PFT_SNAP_DIRECT   2
#define PFT_SNAP_STAGED   4
#define PFT_SNAP_VERSION(v) (((v) & 3) << 8)
#define PFT_SNAP_LINK_DEFAULT PFT_SNAP_LINK_STAGED
int pft_solver_snapshot_write(const char * path, const double * param, const pft_snapshot_info * info, int flags);
int pft_solver_snapshot_wait(void);
/* f11: a region dataset (pft_io.h: pft_region, pft_snapshot_create_region) of the device-resident
   x: the flags, the validity rules and the codes of pft_solver_snapshot_write (-3 without a
   resident state, nothing created; -2 from a Service_Callback with several ranks), and -2 on every
   rank for a bad region, before any file or device work.  Collective: rank 0 writes the header
   even when its slab owns no selected plane, the status allreduce is the barrier, every rank
   exports its share (pft_region_local, pft_slab_region_export) and hands it to the background
   writer; a rank that owns none takes part in every collective and queues no write.
   pft_solver_snapshot_wait covers these writes.
   pft_solver_region: this rank's share of the region (kcount * count[1] * count[0] doubles per
   field, u, p, gl in turn; pft_region_image_bytes of the slab's grid) into out_native in the
   host's byte order, no file: the region image through the pinned buffer, swapped back on the
   host.  Not collective.  The same validity rules; out_native may be NULL when the share is
   empty. */
int pft_solver_snapshot_region_write(const char * path, const double * param, const pft_snapshot_info * info,
                                     const pft_region * region, int flags);
int pft_solver_region(const pft_region * region, double * out_native);
/* f7 (after RK_MPI_SA_init): the state of a snapshot dataset read on the device, as a restart
   (icond_file, intertrack.c:2023-2117): each rank preads only its own planes -- no distribution
   through a master -- and imports them into X and XN (pft_slab_import_be); then exactly the end of
   the device ICs: outcome agreed across ranks, ghost planes exchanged, gl_keep set, the state
   resident.  system->x is not written (pft_solver_download).  -4 on every rank, before any device
   work, when the dataset's dimensions differ from the grid's; other codes as pft_io.h and
   pft_solver_ic_default_device.  pft_solver_ic_beads_device overlays the glass beads on the gl of
   the resident state, as PrecalculateData does for a state from a file (equation.c:507-530). */
int pft_solver_snapshot_read(const char * path);
int pft_solver_ic_beads_device(void);

/* RK_MPI_SA_solve / pft_solve_ex return value added to the reference's codes
   (RK_MPI_SAsolver.h:384-392): a HIP or RCCL failure (out of device memory, a device fault, a
   lost peer).  pft_solver_last_status() gives the raw status (-1000 - hipError_t, -3000 -
   ncclResult_t, -1 host allocation) and pft_hip_last_error() the HIP error text. */
#define PFT_SOLVE_DEVICE_ERROR  (-7)
int pft_solver_last_status(void);

enum {
	PFT_OPT_GL_STATIC = 1,  /* 1: exploit dgl == 0 (equation.c:731,874): gl neither stored in K
	                           nor combined -- bit-identical results, less traffic. Default 0. */
	PFT_OPT_KZ = 2,         /* planes per workgroup z-march; 0 (default) = automatic: the z-chunk
	                           cost model of pft_slab_set_kz */
	PFT_OPT_DEVICE = 3,     /* HIP device of this thread's slab (default: current device) */
	PFT_OPT_TIMING = 4,     /* N > 0: time the stages of every N-th attempted step with HIP events
	                           (stats.stage_ms / stage_n); each timed stage adds ~3 us of
	                           event-packet overhead, so benchmarks sample (N = 10) */
	PFT_OPT_TILE = 5,       /* stage kernel: 1 (default) = automatic, 2 = LDS-tiled at any size with
	                           the automatic tile, 32 / 16 = LDS-tiled 64x8 / 32x16 tiles, 0 =
	                           cache-based kernel (pft_slab_set_tile) */
	PFT_OPT_RECOMPUTE = 6,  /* 1 (default): rebuild stage inputs from x and the K's inside the
	                           stencil, 0: materialise the aux arrays (pft_slab_set_recompute) */
	/* 7, 8: retired (the two-stream / comm-boundary N > 1 orders and the z-wavefront stage
	   schedule, measured slower: DESIGN.md section 8) */
	PFT_OPT_LAZY_ALLOC = 9, /* 1: RK_MPI_SA_init only checks its arguments and the device buffers
	                           are allocated by the first solve (host-only checks of the ABI);
	                           0 (default): RK_MPI_SA_init allocates them, as hybrid2.c:101-112
	                           allocates K1..K5 and aux, and returns -1 when that fails */
	PFT_OPT_PAIR = 10       /* stages 2+3 and 4+5 as pair kernels (pft_slab_pair: stage A evaluated
	                           inside stage B's stencil, never stored -- 21 instead of 39 doubles
	                           per cell-step, bit-identical): 1 (default) = on slabs of at least
	                           4 Ki cells per CU (1 M cells on MI355X), 2 = on any slab they fit,
	                           0 = one launch per stage */
	,
	PFT_OPT_FAIL_RHS = 11,  /* test hook: N > 0 makes the N-th device evaluation of libpft's own
	                           right-hand side on a host array (f_generic_model01/2 called by the
	                           host-staged path) fail as a device fault would; 0 (default) off */
	PFT_OPT_GATE = 12       /* gated steps (f4): 1 = on one slab with one launch per stage and no
	                           Service_Callback, the next attempted step's launches are enqueued
	                           before this step's error norm is read and run on the device's step
	                           decision, which the host checks bit for bit (pft_slab_gate_*);
	                           0 (default) = off: measured neutral at 100^3 (38.2 vs 37.4-38.5 us
	                           per attempted step) and -2% at 200^3, where the step is bound by its
	                           kernels, not by the host.  Bit-identical. */
};
int pft_solver_set_option(int opt, long value);

typedef struct {
	int path;               /* 0 none yet, 1 fused device path, 2 host-staged path */
	int nprocs, rank;
	long kernel_launches;   /* stage kernels launched by the last call */
	long steps_total;       /* attempted steps of the last call */
	double last_eps;        /* max error norm of the last attempted step */
	double stage_ms[6];     /* PFT_OPT_TIMING: summed HIP-event time of stages 1..5 */
	long stage_n[6];        /* number of timed stage executions */
	int pairs;              /* 1: the last fused call ran stages 2+3 and 4+5 as pair kernels
	                           (timed as stages 3 and 5) */
	long gated_steps;       /* attempted steps of the last call that ran as pre-enqueued gated
	                           launches (PFT_OPT_GATE) */
	long gate_misses;       /* ... that were discarded because the device's step size differed
	                           from the host's in the last bit (pow) and were launched again */
} pft_solver_stats;
int pft_solver_get_stats(pft_solver_stats * st);

/* the slab of the fused path (benchmarks / profilers); NULL before the first fused solve */
pft_slab * pft_solver_slab(void);

#ifdef __cplusplus
}
#endif
#endif
