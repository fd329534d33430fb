/*
 * rk_solver.c -- libpft's RK_MPI_SAsolver ABI (include/RK_MPI_SAsolver.h): the adaptive
 * 4th-order Runge-Kutta-Merson solver of modules/RK_MPI_SAsolver_hybrid2/RK_MPI_SAsolver_hybrid2.c
 * (and its twin _hybrid), re-designed for MI355X.
 *
 * Host C.  The control logic -- step size, accept/reject, finish/next-finish, NaN retries,
 * service callback, meta-pointer refresh, return codes -- is restated line for line from
 * hybrid2.c:215-770 (citations inline); every decision uses the same fp64 expressions, so
 * trajectories are identical to the reference's.  The array work runs on the GPU:
 *
 *  - fused path (the hot path): when meta_f() returns libpft's intertrack right-hand side and
 *    the chunk table is the driver's canonical one (intertrack.c:2144-2157), x lives on the
 *    device and each attempted step is 5 fused stage kernels (pft_kernels.hip) + one 16-byte
 *    device->host read of the global error norm; with several ranks the stage outputs' boundary
 *    planes travel by RCCL while the interior planes are computed (pft_comm.h).
 *  - host-staged path: any other RK_RightHandSide is called on the host with host arrays; the
 *    stage combines, the error norm and the update run as HIP kernels over the chunk table.
 *
 * Solver state is per host thread (the reference's is per MPI process: one static instance).
 */
#include "pft_internal.h"
#include "pft_stepctl.h"
#include "../../include/pft_frontend.h"
#include "../../include/pft_formula.h"
#include "../../include/pft_hist.h"
#include "../../include/pft_map.h"

#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef struct {
	int max_n;                    /* hybrid2.c:61; 0 = not initialised */
	int master;
	int handle_nan, last_nan;     /* :63-64 */
	pft_comm * self_comm;
	/* fused path */
	pft_slab * slab;
	pft_grid slab_grid;
	int slab_gls, slab_dev;
	int device_valid;             /* slab X holds the solution left by the previous call */
	/* host-staged path */
	double *d_x, *d_k1, *d_k3, *d_k4, *d_k5, *d_aux, *d_eps;
	int *d_cs, *d_cz; double * d_cm; int d_nch, d_cap;
	double *h_k, *h_aux; int h_cap;
	/* options */
	int opt_gls, opt_kz, opt_dev, opt_timing, opt_tile, opt_norecompute;
	int opt_lazy;               /* PFT_OPT_LAZY_ALLOC: device buffers at the first solve, not at init */
	int opt_pair;               /* PFT_OPT_PAIR: stages 2+3 and 4+5 as pair kernels where the slab can */
	int opt_gate;               /* PFT_OPT_GATE: gated steps on small single slabs (f4) */
	/* K1 = f(t, x) left on the device by the last fused call (its speculative stage 1, swapped in
	   on the last accepted step, or the current one after a rejection): the next call that keeps
	   x resident from the same t, with the same constants and no u_noise, starts at stage 2 */
	int k1_keep;
	double k1_t;
	pft_consts k1_c;
	pft_slab * k1_slab;
	int k1_deep;                /* ... and its far ghost planes are current: the call that left it ran
	                               the deep (pair, between slabs) exchange, not one launch per stage */
	int deep;                   /* this call runs the pair kernels on z-neighbouring slabs: every stage
	                               launch covers the whole slab and is followed by the two-plane halo
	                               exchange of its output (pft_comm_halo_deep) */
	int tstep;                  /* this attempted step's stages are timed (every opt_timing-th) */
	int last_status;            /* raw status of the last device / communication failure */
	int in_callback;            /* inside Service_Callback on the fused path (x is on the device) */
	int rhs_failed;             /* sticky: a device evaluation of libpft's RHS on a host array failed
	                               (f_generic_model01/2 cannot report it: the reference's f is void);
	                               the host-staged loop checks it after every f() */
	long fail_rhs_after, rhs_calls;   /* PFT_OPT_FAIL_RHS test hook */
	pft_solver_stats stats;
} solver_state;

static __thread solver_state R = { .slab_dev = -1, .opt_kz = 0, .opt_dev = -1, .opt_tile = 1, .opt_pair = 1, .opt_gate = 0 };

static pft_comm * comm(void)
{
	pft_comm * c = pft_comm_current();
	if(c) return c;
	if(!R.self_comm) pft_comm_init_self(&R.self_comm);
	return R.self_comm;
}

/* ---------------------------------------------------------------------------------------- */
/* lifecycle, hybrid2.c:72-212 */

static int ensure_slab(void);
static int alloc_staged(void);
static void free_staged(void);

/* the device buffers RK_MPI_SA_init allocates (hybrid2.c:101-112 allocates K1, K3, K4, K5, aux):
   the fused path's slab when the model is configured and max_block_size holds its intertrack
   block (intertrack.c:2192 passes 3 * subgridSIZE), otherwise the host-staged path's arrays */
static int alloc_at_init(void)
{
	pft_grid g;
	int rc;
	if(pft_model_get_grid(&g) == 0) {
		const long S = (g.n1 + 2L*PFT_BCOND_THICKNESS) * (g.n2 + 2L*PFT_BCOND_THICKNESS) *
		               (g.n3 + 2L*PFT_BCOND_THICKNESS);
		if(R.max_n >= PFT_VAR_COUNT*S) return ensure_slab();
	}
	rc = alloc_staged();
	return rc;
}

int RK_MPI_SA_init(int max_block_size, MPI_Comm comm_handle, int master_rank)
{
	pft_comm * c = comm();
	int rc;
	/* :95; the ranks are those of the pft communicator (pft_comm.h), which stands for the
	   driver's MPI_COMM_WORLD -- any other communicator is unknown to libpft */
	if(!c || comm_handle != PFT_COMM_WORLD) return -4;
	if(R.max_n) return -3;                                  /* :98 */
	if(max_block_size <= 0) return -2;                      /* :99 */
	if(master_rank < 0 || master_rank >= pft_comm_size(c)) return -4;
	R.max_n = max_block_size;                               /* :114-118 */
	R.last_nan = 0;
	R.master = master_rank;
	if(!R.opt_lazy && (rc = alloc_at_init())) {             /* :101-112: -1, not enough memory */
		R.last_status = rc;
		if(R.slab) { pft_comm_attach(comm(), NULL); pft_slab_destroy(R.slab); R.slab = NULL; R.k1_keep = 0; }
		free_staged();
		R.max_n = 0;
		return -1;
	}
	return 0;
}

static void free_staged(void)
{
	pft_flat_free(R.d_x); pft_flat_free(R.d_k1); pft_flat_free(R.d_k3); pft_flat_free(R.d_k4);
	pft_flat_free(R.d_k5); pft_flat_free(R.d_aux); pft_flat_free(R.d_eps);
	pft_dev_free(R.d_cs); pft_dev_free(R.d_cz); pft_flat_free(R.d_cm);
	R.d_x = R.d_k1 = R.d_k3 = R.d_k4 = R.d_k5 = R.d_aux = R.d_eps = R.d_cm = NULL;
	R.d_cs = R.d_cz = NULL; R.d_cap = 0; R.d_nch = 0;
	free(R.h_k); free(R.h_aux); R.h_k = R.h_aux = NULL; R.h_cap = 0;
}

int RK_MPI_SA_cleanup(void)
{
	if(R.max_n == 0) return -3;                             /* :130 */
	if(R.slab) { pft_comm_attach(comm(), NULL); pft_slab_destroy(R.slab); R.slab = NULL; R.k1_keep = 0; }
	free_staged();
	R.device_valid = 0;
	R.max_n = 0;                                            /* :134 */
	return 0;
}

void RK_MPI_SA_handle_NAN(int hN) { R.handle_nan = (hN == 0) ? 0 : 1; }   /* :165 */
int RK_MPI_SA_check_NAN() { return R.last_nan; }                           /* :176 */

int RK_MPI_SA_check_mem(RK_MEM_DIST * n)
{
	/* :191-211 */
	int offset = 0, prev, i;
	if(R.max_n == 0) return -3;
	if(n->n_chunks <= 0) return -7;
	for(i=0;i<n->n_chunks;i++) {
		prev = offset;
		offset = n->chunk_start[i];
		if(offset < prev) return -6;
		prev = offset;
		offset += n->chunk_size[i];
		if(offset <= prev) return -6;
	}
	if(offset > R.max_n) return -5;
	return 0;
}

int pft_solver_set_option(int opt, long value)
{
	switch(opt) {
		case PFT_OPT_GL_STATIC: R.opt_gls = value ? 1 : 0; return 0;
		case PFT_OPT_KZ: if(value < 0) return -2; R.opt_kz = (int)value; if(R.slab) pft_slab_set_kz(R.slab, R.opt_kz); return 0;
		case PFT_OPT_DEVICE: R.opt_dev = (int)value; return 0;
		case PFT_OPT_TIMING: if(value < 0) return -2; R.opt_timing = (int)value; return 0;
		case PFT_OPT_LAZY_ALLOC: R.opt_lazy = value ? 1 : 0; return 0;
		case PFT_OPT_FAIL_RHS: if(value < 0) return -2; R.fail_rhs_after = value; R.rhs_calls = 0; return 0;
		case PFT_OPT_PAIR: if(value < 0 || value > 2) return -2; R.opt_pair = (int)value; return 0;
		case PFT_OPT_GATE: if(value < 0 || value > 1) return -2; R.opt_gate = (int)value; return 0;
		case PFT_OPT_RECOMPUTE:
			R.opt_norecompute = value ? 0 : 1; if(R.slab) pft_slab_set_recompute(R.slab, !R.opt_norecompute); return 0;
		case PFT_OPT_TILE:
			if(value != 0 && value != 1 && value != 2 && value != 16 && value != 32) return -2;
			R.opt_tile = (int)value; if(R.slab) pft_slab_set_tile(R.slab, R.opt_tile); return 0;
	}
	return -2;
}

int pft_solver_get_stats(pft_solver_stats * st) { *st = R.stats; return 0; }
int pft_solver_last_status(void) { return R.last_status; }
pft_slab * pft_solver_slab(void) { return R.slab; }

/* ---------------------------------------------------------------------------------------- */
/* fused device path */

static int ensure_slab(void)
{
	pft_grid g;
	pft_consts c;
	pft_slab_desc d;
	int rc;
	if(pft_model_get_grid(&g) || pft_model_get_consts(&c)) return -2;
	if(R.slab && R.slab_grid.n1 == g.n1 && R.slab_grid.n2 == g.n2 && R.slab_grid.n3 == g.n3 &&
	   R.slab_grid.rank == g.rank && R.slab_grid.nprocs == g.nprocs && R.slab_grid.calc_mode == g.calc_mode &&
	   R.slab_gls == R.opt_gls && R.slab_dev == R.opt_dev) {
		/* parameters may change between calls: refresh the constants */
		pft_slab_set_consts(R.slab, &c);
	} else if(R.slab) {
		pft_comm_attach(comm(), NULL);
		pft_slab_destroy(R.slab); R.slab = NULL; R.device_valid = 0; R.k1_keep = 0;
	}
	if(!R.slab) {
		if(R.opt_dev >= 0 && (rc = pft_hip_set_device(R.opt_dev))) return rc;
		memset(&d, 0, sizeof(d));
		d.n1 = g.n1; d.n2 = g.n2; d.n3 = g.n3;
		d.has_below = g.rank > 0;
		d.has_above = g.rank < g.nprocs - 1;
		d.calc_mode = g.calc_mode;
		d.gl_static = R.opt_gls;
		d.eps_mult[0] = d.eps_mult[1] = d.eps_mult[2] = 1.0;
		if((rc = pft_slab_create(&R.slab, &d, &c))) return rc;
		pft_slab_set_kz(R.slab, R.opt_kz);
		pft_slab_set_tile(R.slab, R.opt_tile);
		pft_slab_set_recompute(R.slab, !R.opt_norecompute);
		R.slab_grid = g; R.slab_gls = R.opt_gls; R.slab_dev = R.opt_dev;
		R.device_valid = 0;
	}
	if((rc = pft_comm_attach(comm(), R.slab))) return rc;
	return pft_slab_set_noise(R.slab, pft_model_noise());
}

static int canonical_chunks(const RK_MEM_DIST * n, double em[3])
{
	/* the intertrack chunk table (intertrack.c:2144-2157) for the configured grid */
	pft_grid g;
	int q, k, j, c = 0;
	long N1, row, S;
	if(pft_model_get_grid(&g)) return 0;
	N1 = g.n1 + 2*PFT_BCOND_THICKNESS; row = N1*(g.n2 + 2*PFT_BCOND_THICKNESS);
	S = row*(g.n3 + 2*PFT_BCOND_THICKNESS);
	if(n->n_chunks != PFT_VAR_COUNT*g.n2*g.n3) return 0;
	for(q=0;q<PFT_VAR_COUNT;q++) {
		em[q] = n->chunk_eps_mult ? n->chunk_eps_mult[c] : 1.0;
		for(k=0;k<g.n3;k++) for(j=0;j<g.n2;j++, c++) {
			const long s0 = q*S + (k+PFT_BCOND_THICKNESS)*row + (long)(j+PFT_BCOND_THICKNESS)*N1 + PFT_BCOND_THICKNESS;
			if(n->chunk_start[c] != s0 || n->chunk_size[c] != g.n1) return 0;
			if(n->chunk_eps_mult && n->chunk_eps_mult[c] != em[q]) return 0;
		}
	}
	return R.max_n >= PFT_VAR_COUNT*S;
}

/* what place() launches: one stage of the step (t, h) on this slab (stage 1..5; 6 = the speculative
   stage 1 of the next step, K1' = f(t+h, XN) into A1, pft_slab_stage_spec), or stages first, first+1 (2+3
   or 4+5) as ONE pair kernel (pft_slab_pair); the scalars are the step controller's */
typedef struct { int stage, first; double t, h; } launch_what;

static int run1(const launch_what * w, int kb, int ke)
{
	const pft_stage_scalars s = pft_stepctl_stage(w->first ? w->first : w->stage, w->t, w->h);
	if(w->first)   /* (coef: x(t+h)'s, stage 5's, for either pair, as the pair kernel takes it) */
		return pft_slab_pair_range(R.slab, w->first, s.ts, pft_stepctl_stage(w->first+1, w->t, w->h).ts, w->h,
		                           pft_stepctl_stage(5, w->t, w->h).coef, kb, ke);
	return w->stage == 6 ? pft_slab_stage_spec(R.slab, s.ts, kb, ke) : pft_slab_stage(R.slab, w->stage, s.ts, s.coef, w->h, kb, ke);
}

/* a launch and the exchange of its output's boundary planes (nfields fields of out_buf), timed as
   stage tstage */
static int place(const launch_what * w, int out_buf, int nfields, int tstage, long * launches)
{
	pft_comm * c = comm();
	/* boundary first: the transport splits, and is not ipc with put kernels */
	const int n3 = R.slab_grid.n3, bf = pft_comm_boundary_first(c);
	int rc, depth = 0, inl = 0;   /* planes at each end of a split launch's boundary; an inline boundary's code */
	if(R.tstep) pft_slab_timing_mark(R.slab, tstage, 0);
	if(R.deep && bf && n3 >= 5) {
		/* pair path between slabs over RCCL or the copy engines: the output's two-plane halo (the next
		   pair kernel evaluates its stage A on the ghost planes too; K3, or x(t+h): gl only where
		   stored) -- the two planes at each end first, their exchange on the comm stream beside the
		   interior launch, which reads no ghost plane; or (inl) one launch whose leading workgroups
		   produce those planes, the copies starting when they are done (PFT_K_INLINE, PFT_K_ENDS_FIRST) */
		depth = 2;
		inl = w->first ? pft_slab_pair_inline(R.slab, w->first) : pft_slab_stage_inline(R.slab);
	} else if(!R.deep && !w->first && bf) {
		/* SURVEY 8e.  Stage s reads the stage-(s-1) values of planes -1..n3 and writes its own; only
		   its two boundary planes read ghost planes: they are launched first, exchanged on the comm
		   stream beside the interior sweep, and the compute stream waits for the exchange before the
		   next stage.  (Measured slower and removed: the boundary launch on the comm stream with the
		   interior sweep waiting for it, and two-stream orders) */
		depth = 1;
	}
	if(depth) {
		*launches += inl ? 1 : 2;
		if((rc = run1(w, inl ? inl : depth == 2 ? PFT_K_BOUNDARY2 : PFT_K_BOUNDARY, 0))) return rc;
		if((rc = depth == 2 ? pft_comm_halo_start_deep(c, out_buf, 0, nfields) : pft_comm_halo_start(c, out_buf, 0, nfields)))
			return rc;
		if(!inl && n3 > 2*depth && (rc = run1(w, depth, n3-depth))) return rc;   /* (depth 2: n3 >= 5) */
		if(R.tstep) pft_slab_timing_mark(R.slab, tstage, 1);
		return pft_comm_halo_finish(c);
	}
	(*launches)++;
	if((rc = run1(w, -1, -1))) return rc;
	if(R.tstep) pft_slab_timing_mark(R.slab, tstage, 1);
	/* ... then, between slabs with put kernels (ipc), stream-ordered: the boundary planes into the
	   neighbours' ghost planes and the wait for theirs in ours (pair path: the two-plane halo) */
	if(R.deep) return pft_comm_halo_deep(c, out_buf, 0, nfields);
	if(!w->first && pft_comm_device_halo(c) && !bf) return pft_comm_halo(c, out_buf, 0, nfields);
	return 0;
}

static int do_stage(int stage, double t, double h, long * launches)
{
	const launch_what w = {stage, 0, t, h};
	return place(&w, stage == 6 ? PFT_BUF_A1 : pft_slab_stage_output(R.slab, stage),
	             pft_slab_stage_fields(R.slab, stage), stage == 6 ? 1 : stage, launches);
}

/* timed as stage first+1 */
static int do_pair(int first, double t, double h, long * launches)
{
	const launch_what w = {0, first, t, h};
	return place(&w, first == 2 ? PFT_BUF_K3 : PFT_BUF_XN, pft_slab_stage_fields(R.slab, first+1), first+1, launches);
}

/* gl evolves by dgl == 0 (equation.c:731,874), so x(t+h) of gl is x + coef*0.0: x itself, bit for
   bit, unless x is -0.0 (-0.0 + 0.0 = +0.0) or NaN.  When no gl value of the uploaded state is
   either, X and XN (both uploaded from it) keep identical gl for good and stage 5 skips that store
   (pft_slab_set_gl_keep); one step turns any -0.0 into +0.0, so the check only looks at input. */
static int gl_clean(const double * x)
{
	/* host layout: [q][k][j][i] with 2 ghost cells on every side; only the interior is uploaded */
	const int n1 = R.slab_grid.n1, n2 = R.slab_grid.n2, n3 = R.slab_grid.n3;
	const long N1 = n1 + 4, N2 = n2 + 4;
	const double * g = x + 2 * N1 * N2 * (n3 + 4);
	int k, bad = 0;
	#pragma omp parallel for reduction(|:bad) schedule(static)
	for(k = 2; k < n3 + 2; k++) {
		int j, i;
		for(j = 2; j < n2 + 2; j++) {
			const double * r = g + ((long)k * N2 + j) * N1;
			for(i = 2; i < n1 + 2; i++) bad |= (r[i] != r[i]) || (r[i] == 0.0 && signbit(r[i]));
		}
	}
	return !bad;
}

/* shared prologue results: the solve's constants and the attempt under way (t, h, the pending command) */
typedef struct { pft_stepctl_consts k; pft_step a; int any_cb; } solve_bcast;

static int run_staged(RK_MPI_S_SOLUTION * system, RK_RightHandSide f, solve_bcast * B, long max_steps_total, int flags);

/* What run_fused and run_staged share around the step controller (pft_stepctl.h): a loop computes the attempt
   B->a its own way, then step_judge, if accepted its own accept action and step_accepted, then step_next */
typedef struct {
	RK_MPI_S_SOLUTION * system;
	solve_bcast * B;
	long max_steps, attempted;
	int command, ret;     /* the attempt as judged, with new_h; the call's return code once a routine ends the loop */
	double new_h;
} step_loop;

/* count and judge the attempt, its error norm known; 1: the solve ends here (-4) */
static int step_judge(step_loop * L, double eps, int nonfinite)
{
	L->system->steps_total++;                                                /* :460 */
	L->attempted++;
	R.stats.last_eps = eps;                                                  /* unscaled by DELTA_LOCAL */
	L->command = pft_stepctl_judge(L->B->k, L->B->a, eps, nonfinite, &L->new_h);
	if(L->command & RKA_CMD_NAN) R.last_nan = 1;                             /* :626-646 */
	if((L->command & RKA_CMD_NAN) && (L->command & RKA_CMD_h_TOO_SMALL)) L->ret = -4;
	return L->ret == -4;
}

/* accepted, x is x(t+h) (resident: on the device): B->a advances; callback, broadcast, FINISHED and BREAK.
   1: the solve ends here; negative: a collective failed */
static int step_accepted(step_loop * L, int resident)
{
	RK_MPI_S_SOLUTION * system = L->system;
	const double h = L->B->a.h;
	int rc;
	L->B->a = pft_stepctl_advance(L->B->k, L->B->a, L->command, L->new_h);
	system->steps++;
	if(system->Service_Callback != NULL) {                                   /* :676-685 */
		system->t = L->B->a.t;
		system->h = h;
		R.in_callback = resident;            /* a callback that reads x calls pft_solver_download first */
		if(system->Service_Callback(L->B->k.final_time, system)) L->command |= RKA_CMD_BREAK;
		R.in_callback = 0;
	}
	if(pft_comm_size(comm()) > 1 && L->B->any_cb && (rc = pft_comm_bcast(comm(), &L->command, sizeof(int), R.master)))
		return rc;                                                           /* :690 */
	if(L->command & RKA_CMD_FINISHED) return 1;                              /* :695 */
	if(!(L->command & RKA_CMD_BREAK)) return 0;
	system->h = L->new_h;                                                    /* :697-705 */
	L->ret = 1;
	return 1;
}

/* on to the next attempt (:743-761; an accepted one has advanced).  1: the step cap (an extension) ends the
   call between two attempts; the next call's prologue re-derives FINISHED from t, h */
static int step_next(step_loop * L)
{
	if(!pft_stepctl_accepted(L->command)) L->B->a = pft_stepctl_advance(L->B->k, L->B->a, L->command, L->new_h);
	else if(L->command & RKA_CMD_NEXTFINISH) L->system->h = L->new_h;
	if(!(L->max_steps > 0 && L->attempted >= L->max_steps)) return 0;
	L->system->h = L->B->a.h;
	L->ret = 2;
	return 1;
}

/* PFT_GATE_TRACE=1: host-side timeline of the gated pipeline (stderr at the end of a call) */
static double gt_now(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

static int run_fused(RK_MPI_S_SOLUTION * system, RK_RightHandSide f, solve_bcast * B, long max_steps_total,
                     int flags, const double * em)
{
	pft_comm * c = comm();
	const int nprocs = pft_comm_size(c);
	step_loop L = {system, B, max_steps_total};
	double eps;
	int nonfinite, rc, st, to_host = 0;
	long launches = 0;
	int spec, k1_valid = 0;               /* K1 holds f(t, x) for the current t and x */
	int pair;                             /* stages 2+3 and 4+5 as pair kernels */
	int gate, pre = 0, acc, enq;          /* gated steps; this attempt was pre-enqueued; accepted;
	                                         the next attempt is pre-enqueued */
	unsigned long long gcur = 0, gnext;   /* decisions on this attempt (by its speculative stage 1)
	                                         and on the pre-enqueued one */

	if((rc = ensure_slab())) return rc;
	pft_slab_set_eps_mult(R.slab, em);
	/* The next step's K1 is computed speculatively right after stage 5 (recompute path): the
	   kernel runs while the host reads the error norm and decides, so the GPU does not idle
	   between steps.  Accepted: it is f(t+h, x(t+h)), exactly the next stage 1.  Rejected: x and t
	   are unchanged, so the current K1 is still exactly f(t, x) -- the reference recomputes the
	   same bits (hybrid2.c:373) -- and the speculative one is dropped. */
	spec = pft_slab_can_speculate(R.slab);
	/* pair kernels (pft_slab_pair_ok: slab size, n3 >= 2 and no u_noise between slabs); every rank
	   must take the same path -- the exchanges differ */
	pft_slab_set_pair(R.slab, R.opt_pair);
	pair = spec && pft_slab_pair_ok(R.slab);
	if(nprocs > 1) {
		long long no = !pair;
		if((rc = pft_comm_allreduce_max_i64(c, &no))) return rc;
		pair = !no;
	}
	R.deep = pair && pft_comm_splits(c);
	{
		/* K1 from the previous call (R.k1_keep): x resident and unchanged since (no upload), the
		   same slab, t, constants, and no u_noise (re-uploaded every call); for the pair kernels
		   between slabs also its far ghost planes (R.k1_deep: a call with one launch per stage
		   exchanged only the first ghost plane, and the deep prologue below re-exchanges only X
		   and XN).  Every rank takes the same decision (the same calls, flags and t). */
		pft_consts cc;
		if(spec && (flags & PFT_SOLVE_REUSE_DEVICE) && R.device_valid && R.k1_keep && R.k1_slab == R.slab &&
		   (!R.deep || R.k1_deep) && !pft_model_noise() && memcmp(&R.k1_t, &B->a.t, sizeof R.k1_t) == 0 && !pft_model_get_consts(&cc) &&
		   memcmp(&cc, &R.k1_c, sizeof cc) == 0)
			k1_valid = 1;
		R.k1_keep = 0;
	}
	R.stats.pairs = pair;
	R.stats.gated_steps = 0;
	R.stats.gate_misses = 0;
	if(!(flags & PFT_SOLVE_REUSE_DEVICE) || !R.device_valid) {
		if((rc = pft_slab_upload_host(R.slab, PFT_BUF_X, system->x))) return rc;
		if((rc = pft_slab_upload_host(R.slab, PFT_BUF_XN, system->x))) return rc;
		{
			/* every rank must agree: the stage-5 exchange carries gl only when some rank stores it */
			long long unclean = !gl_clean(system->x);
			if(nprocs > 1 && (rc = pft_comm_allreduce_max_i64(c, &unclean))) return rc;
			pft_slab_set_gl_keep(R.slab, !unclean);
		}
		if(nprocs > 1 && !R.deep) {
			if((rc = pft_comm_halo(c, PFT_BUF_X, 0, 3))) return rc;
			if((rc = pft_comm_halo(c, PFT_BUF_XN, 0, 3))) return rc;
		}
	}
	if(R.deep) {
		/* two planes deep, also when x stayed on the device (the previous call may have run one
		   launch per stage, which keeps only the first ghost plane current) */
		if((rc = pft_comm_halo_deep(c, PFT_BUF_X, 0, 3))) return rc;
		if((rc = pft_comm_halo_deep(c, PFT_BUF_XN, 0, 3))) return rc;
	}
	R.device_valid = 0;
	R.stats.path = 1;
	/* the error norm goes to the host from stage 5 itself (no publish kernel, no event) where no
	   device collective sits between stage 5 and the host (one slab, or ipc); env
	   PFT_INKERNEL_PUBLISH=0 turns it off (A/B) */
	{
		const char * e = getenv("PFT_INKERNEL_PUBLISH");
		const int on = spec && (!pft_comm_splits(c) || pft_comm_device_halo(c)) &&
		               !(e && atoi(e) == 0);
		pft_slab_set_inkernel_publish(R.slab, on);
	}

	/* f4, gated steps (PFT_OPT_GATE, pft_slab_gate_*): on one slab with one launch per stage, the
	   next attempted step's launches are enqueued before this step's error norm is read, as if the
	   step were accepted.  This step's speculative stage 1 reduces the error norm and decides the
	   step on the device (the controller of pft_stepctl.h, as step_judge here); the gated launches run on
	   that decision, so the GPU waits neither for the host's round trip nor for its launch latency.
	   The host still takes its own decision (glibc pow) and keeps the gated step only if the
	   device's (ocml pow) is the same bit for bit; otherwise that step is discarded -- it wrote only
	   buffers nothing reads afterwards (XN, A0, K3, K4, A1) -- and launched again.  Not with a
	   Service_Callback (it may read x between steps) or per-stage timing. */
	{
		/* env PFT_GATE=0/1 overrides PFT_OPT_GATE (whole-suite runs with gating forced on) */
		const char * eg = getenv("PFT_GATE");
		gate = eg ? atoi(eg) != 0 : R.opt_gate;
	}
	gate = gate && spec && !pair && nprocs == 1 && !pft_comm_splits(c) &&
	       system->Service_Callback == NULL && !R.opt_timing;
	if(gate) pft_slab_gate_config(R.slab, B->k.final_time, B->k.delta, B->k.h_min, B->k.delta_local, B->k.handle_nan);
	const int gtrace = getenv("PFT_GATE_TRACE") != NULL;
	double gt_t0 = 0.0, gt_enq = 0.0, gt_wait = 0.0, gt_dec = 0.0, gt_a, gt_b;
	long gt_n = 0;
	if(gtrace) gt_t0 = gt_now();

	while(1) {
		const double t = B->a.t, h = B->a.h;
		R.tstep = R.opt_timing > 0 && L.attempted % R.opt_timing == 0;
		acc = 0;
		if(!pre) {
			/* the error norm accumulator is reset by its publication on the speculative path */
			if((!spec || L.attempted == 0) && (rc = pft_slab_eps_reset(R.slab))) return rc;
			/* K1 = f(t,x); aux = x + K1 h/3 ... K5 = f(t+h, aux); error norm; x(t+h) candidate */
			if(pair) {
				/* the same arithmetic: stage A of each pair is evaluated inside stage B's stencil */
				if(!k1_valid && (rc = do_stage(1, t, h, &launches))) return rc;          /* :373-389 */
				if((rc = do_pair(2, t, h, &launches))) return rc;                        /* :392-429 */
				if((rc = do_pair(4, t, h, &launches))) return rc;                        /* :432-524,657-668 */
			} else {
				if(!(spec && k1_valid) && (rc = do_stage(1, t, h, &launches))) return rc;  /* :373-389 */
				for(st = 2; st <= 5; st++)                                   /* :392-453,507-524,657-668 */
					if((rc = do_stage(st, t, h, &launches))) return rc;
			}
			k1_valid = 1;
			if(spec) {
				/* eps max over ranks (:572) and its publication beside the speculative stage 1 */
				if((rc = pft_comm_eps_publish(c))) return rc;
				if(gate) gcur = pft_slab_gate_arm(R.slab, t, h);
				if((rc = do_stage(6, t, h, &launches))) return rc;
			} else {
				/* the boundary launch of stage 5 (comm stream) adds to the error norm too */
				if(pft_comm_splits(c) && (rc = pft_slab_order(R.slab, 1))) return rc;
				if((rc = pft_comm_allreduce_eps(c))) return rc;                      /* :572 */
			}
		}
		pre = 0;
		gnext = 0;
		gt_a = gtrace ? gt_now() : 0.0;
		/* pre-enqueue the next attempt unless this one ends the solve if accepted (FINISHED) or the
		   step cap stops before it */
		enq = gate && gcur && !(B->a.command & RKA_CMD_FINISHED) &&
		      !(max_steps_total > 0 && L.attempted + 1 >= max_steps_total);
		if(enq) {
			/* the next attempted step, enqueued now as if this one were accepted (the buffers
			   swapped as the accept below swaps them, for the enqueue only): stages 2-5 and its
			   speculative stage 1, gated on the device's decision gcur.  The scalars passed here
			   are not used: the launches derive theirs from the decided (t, h). */
			pft_slab_book_save(R.slab, 0);
			pft_slab_accept(R.slab);
			pft_slab_swap_buffers(R.slab, PFT_BUF_K1, PFT_BUF_A1);
			pft_slab_gate_use(R.slab, gcur);
			for(rc = 0, st = 2; st <= 5 && !rc; st++) rc = do_stage(st, 0.0, 0.0, &launches);
			if(!rc) rc = pft_comm_eps_publish(c);
			if(!rc) gnext = pft_slab_gate_arm(R.slab, 0.0, 0.0);   /* (t, h) from its own gate */
			if(!rc) rc = do_stage(6, 0.0, 0.0, &launches);
			pft_slab_gate_use(R.slab, 0);
			pft_slab_accept(R.slab);
			pft_slab_swap_buffers(R.slab, PFT_BUF_K1, PFT_BUF_A1);
			pft_slab_book_save(R.slab, 1);
			pft_slab_book_load(R.slab, 0);
			if(rc) return rc;
		}
		gt_b = gtrace ? gt_now() : 0.0;
		if((rc = pft_slab_eps_fetch(R.slab, &eps, &nonfinite))) return rc;
		if(gtrace) {
			const double n = gt_now();
			gt_enq += gt_b - gt_a;
			gt_wait += n - gt_b;
			gt_a = n;
			gt_n++;
		}
		if((rc = pft_comm_eps_host(c, &eps, &nonfinite))) return rc;                 /* :572 (ipc) */
		if(R.opt_timing) pft_slab_timing_collect(R.slab, R.stats.stage_ms, R.stats.stage_n);
		if(step_judge(&L, eps, nonfinite)) break;
		if(pft_stepctl_accepted(L.command)) {                                             /* :651-668 */
			acc = 1;
			pft_slab_accept(R.slab);
			if(spec) pft_slab_swap_buffers(R.slab, PFT_BUF_K1, PFT_BUF_A1);      /* K1 = f(t, x) */
			else k1_valid = 0;
			if((rc = step_accepted(&L, 1)) < 0) return rc;
			if(rc) break;
			f = system->meta_f();                                                /* :732 */
			/* another right-hand side from the next step on: the state leaves the device
			   and the loop continues on the host-staged path (below) */
			if(!pft_model_is_device_rhs(f)) to_host = 1;
		}
		if(step_next(&L)) break;
		if(to_host) break;
		if(enq) {
			/* keep the pre-enqueued attempt iff the device took this decision, bit for bit:
			   accepted, and the same next t and h (its launches ran on them); otherwise it
			   exited at once (device: rejected) or ran on a different h (pow) and is discarded */
			int go = 0;
			double td = 0.0, hd = 0.0;
			if((rc = pft_slab_gate_decision(R.slab, gcur, &go, &td, &hd))) return rc;
			if(gtrace) gt_dec += gt_now() - gt_a;
			if(acc && go && memcmp(&td, &B->a.t, sizeof td) == 0 && memcmp(&hd, &B->a.h, sizeof hd) == 0) {
				pft_slab_book_load(R.slab, 1);
				pre = 1;
				R.stats.gated_steps++;
				gcur = gnext;
			} else {
				if(acc && go) R.stats.gate_misses++;
				gcur = 0;
			}
		} else {
			gcur = 0;
		}
	}
	if(gtrace && gt_n)
		fprintf(stderr, "libpft gate trace: %ld attempts, %.2f us each: enqueue %.2f, eps wait %.2f, "
		        "decide+compare %.2f (gated %ld, pow misses %ld)\n", gt_n, (gt_now() - gt_t0) / gt_n,
		        gt_enq / gt_n, gt_wait / gt_n, gt_dec / gt_n, R.stats.gated_steps, R.stats.gate_misses);
	/* join the comm stream (the last boundary launch and exchange) before the state leaves */
	if(pft_comm_splits(c) && (rc = pft_slab_order(R.slab, 1))) return rc;
	system->t = B->a.t;                                                             /* :768 */
	if(spec && k1_valid && L.ret != -4 && !to_host && !pft_model_get_consts(&R.k1_c)) {
		/* K1 = f(t, x) for the state this call leaves on the device (see R.k1_keep) */
		R.k1_keep = 1;
		R.k1_t = B->a.t;
		R.k1_slab = R.slab;
		R.k1_deep = R.deep;
	}
	if(R.opt_timing) pft_slab_timing_flush(R.slab, R.stats.stage_ms, R.stats.stage_n);
	R.tstep = 0;
	R.device_valid = 1;
	R.stats.kernel_launches = launches;
	R.stats.steps_total = L.attempted;
	if(!(flags & PFT_SOLVE_KEEP_DEVICE) || to_host) {
		if((rc = pft_slab_download_host(R.slab, PFT_BUF_X, system->x))) return rc;
	}
	if(to_host) {
		/* meta_f() returned a right-hand side that is not libpft's: carry on from the attempt B->a with it
		   on the host-staged path (hybrid2.c:732 keeps integrating with the new f) -- unless the step cap
		   ended this call on that very step: then it returns 2 like any capped call, and the next call (its
		   prologue calls meta_f()) takes the host-staged path from the start */
		R.device_valid = 0;
		if(L.ret == 2) return L.ret;
		return run_staged(system, f, B, max_steps_total > 0 ? max_steps_total - L.attempted : 0, flags);
	}
	return L.ret;
}

int pft_solver_download(RK_MPI_S_SOLUTION * system)
{
	if(!R.slab || !(R.device_valid || R.in_callback) || !system || !system->x) return -2;
	return pft_slab_download_host(R.slab, PFT_BUF_X, system->x);
}

#define PFT_DIAG_MAX_RANKS 64   /* the ipc transport's limit (PFT_IPC_MAX) */

/* the rule of every entry that reads the resident state: -3 with no initialised solver or no resident
   state (before the first fused solve with a host IC, the host-staged path, after a failed call): no
   stale numbers.  A collective entry is also -2 inside a Service_Callback with several ranks: only
   one rank may ask there, another rank's callback need not */
static int resident_state(int collective)
{
	if(R.max_n == 0 || !R.slab || !(R.device_valid || R.in_callback)) return -3;
	if(collective && R.in_callback && pft_comm_size(comm()) > 1) return -2;
	return 0;
}

/* a compile outcome as a rank for a max over the ranks, and back: 1 (not device-exact) and -2 (a bad
   program) are the same on every rank, -1 (out of memory) is local; -1 over -2 over 1 over 0 */
static long long compile_rank(int rc)
{
	return rc == -1 ? 3 : (rc == -2 ? 2 : (rc == 1 ? 1 : (rc ? 3 : 0)));
}

static int compile_code(long long v)
{
	return v == 3 ? -1 : (v == 2 ? -2 : (v == 1 ? 1 : 0));
}

/* the ranks agree a compile outcome before anything else collective, so that every rank returns the
   same code (a single rank keeps its own): 0, or the collective's error */
static int compile_agree(int * rc)
{
	long long v = compile_rank(*rc);
	int crc;
	if(pft_comm_size(comm()) == 1) return 0;
	if((crc = pft_comm_allreduce_max_i64(comm(), &v))) return crc;
	*rc = compile_code(v);
	return 0;
}

/* The gather of the four reductions (f5, f6, f12, f13).  `mine` is a {long long status; record}
   message of `used` bytes; every rank sends it whatever its status (a rank that failed locally, or
   whose allocation failed here -- it reports -1 -- still takes part, so that no other rank is left
   inside a collective: pft_comm_allgather_any makes the rounds), and the statuses are judged after
   the rounds.  0 with rank r's message at *all + r*used, to be given to drop_records; or
   PFT_SOLVE_DEVICE_ERROR on every rank, with R.last_status the rank's own non-zero status, otherwise
   the lowest-ranked bad rank's.  A single rank makes no collective and no allocation: *all is mine.
   (Loopback ranks are threads of one process: nothing static.) */
static int gather_records(long long status, void * mine, size_t used, char ** all)
{
	pft_comm * c = comm();
	const int nprocs = pft_comm_size(c);
	int rc = 0, r;
	*all = nprocs == 1 ? (char *)mine : (char *)malloc((size_t)nprocs * used);
	if(!*all && !status) status = -1;
	memcpy(mine, &status, sizeof status);
	if(nprocs > 1 && (rc = pft_comm_allgather_any(c, mine, used, *all))) status = rc;
	for(r = 0; r < nprocs && !status; r++) memcpy(&status, *all + (size_t)r*used, sizeof status);
	if(status) {
		if(*all != (char *)mine) free(*all);
		R.last_status = (int)status;
		return PFT_SOLVE_DEVICE_ERROR;
	}
	return 0;
}

static void drop_records(char * all, const void * mine)
{
	if(all != (const char *)mine) free(all);
}

int pft_solver_diag(const pft_diag_opts * opts, pft_diag * global, pft_diag * local, long long * ice_per_plane)
{
	/* f5: the diagnostics of the device-resident x.  Each rank reduces its slab; the records travel
	   with the rank's status (gather_records: one round) and are merged in rank order, so every rank
	   has the same record and returns the same code */
	struct diag_msg { long long status; pft_diag d; } mine;
	char * all;
	const int nprocs = pft_comm_size(comm());
	int rc, r;
	if(!global) return -2;
	if((rc = resident_state(1))) return rc;
	if(nprocs > PFT_DIAG_MAX_RANKS || sizeof(mine) > 256) return -2;
	memset(&mine, 0, sizeof mine);
	rc = pft_slab_diag(R.slab, PFT_BUF_X, opts, &mine.d, ice_per_plane);
	if((rc = gather_records(rc, &mine, sizeof mine, &all))) return rc;
	*global = ((const struct diag_msg *)all)->d;
	for(r = 1; r < nprocs; r++) pft_diag_combine(global, &((const struct diag_msg *)all)[r].d);
	if(local) *local = mine.d;
	drop_records(all, &mine);
	return 0;
}

int pft_solver_means(const pft_diag_opts * opts, pft_means * global, pft_means * local, pft_means * per_plane)
{
	/* f6: the exact sums of the device-resident x, under pft_solver_diag's rules; the records are
	   merged in rank order: integer sums, the same bits on every rank */
	struct means_msg { long long status; pft_means m; } mine;
	char * all;
	const int nprocs = pft_comm_size(comm());
	int rc, r;
	if(!global) return -2;
	if((rc = resident_state(1))) return rc;
	if(nprocs > PFT_DIAG_MAX_RANKS) return -2;
	memset(&mine, 0, sizeof mine);
	rc = pft_slab_means(R.slab, PFT_BUF_X, opts, &mine.m, per_plane);
	if((rc = gather_records(rc, &mine, sizeof mine, &all))) return rc;
	*global = ((const struct means_msg *)all)->m;
	for(r = 1; r < nprocs; r++) pft_means_combine(global, &((const struct means_msg *)all)[r].m);
	if(local) *local = mine.m;
	drop_records(all, &mine);
	return 0;
}

int pft_solver_formulas(int nprog, const int * lens, const int * ops, const double * args, pft_fdiag * global,
                        pft_fdiag * local, pft_fdiag * per_plane)
{
	/* f12: the formula diagnostics of the device-resident x, under pft_solver_diag's rules.  Every
	   rank compiles first and the outcome is agreed before any device work (compile_agree), as in
	   pft_solver_ic_formulas_device.  Then each rank reduces its slab and the used part of its
	   message travels (gather_records); the records are merged in rank order */
	struct formula_msg { long long status; pft_fdiag d[PFT_FORMULA_MAX]; } mine;
	char * all;
	pft_ic_prog pr[PFT_FORMULA_MAX];
	pft_grid g;
	const int nprocs = pft_comm_size(comm());
	int rc, crc, r, f, off = 0, entries = 0;
	size_t used;
	if(!global) return -2;
	if((rc = resident_state(1))) return rc;
	if(nprocs > PFT_DIAG_MAX_RANKS) return -2;
	if(nprog < 1 || nprog > PFT_FORMULA_MAX || !lens || !ops || !args || pft_model_get_grid(&g)) rc = -2;
	for(f = 0; f < nprog && !rc; f++) {
		if(lens[f] < 1 || (entries += lens[f]) > PFT_FORMULA_MAX_ENTRIES) rc = -2;
	}
	memset(pr, 0, sizeof pr);
	for(f = 0; f < nprog && !rc; f++) {
		rc = pft_formula_compile(&g, lens[f], ops + off, args + off, &pr[f]);
		off += lens[f];
	}
	if((crc = compile_agree(&rc))) {
		R.last_status = crc;
		rc = PFT_SOLVE_DEVICE_ERROR;
	}
	if(rc) {
		for(f = 0; f < PFT_FORMULA_MAX; f++) pft_ic_prog_free(&pr[f]);
		return rc;
	}
	memset(&mine, 0, sizeof mine);
	rc = pft_slab_formulas(R.slab, PFT_BUF_X, nprog, pr, mine.d, per_plane);
	for(f = 0; f < PFT_FORMULA_MAX; f++) pft_ic_prog_free(&pr[f]);
	used = offsetof(struct formula_msg, d) + (size_t)nprog * sizeof(pft_fdiag);
	if((rc = gather_records(rc, &mine, used, &all))) return rc;
	for(f = 0; f < nprog; f++) {
		global[f] = ((const struct formula_msg *)all)->d[f];
		for(r = 1; r < nprocs; r++)
			pft_fdiag_combine(&global[f], &((const struct formula_msg *)(all + (size_t)r*used))->d[f]);
		if(local) local[f] = mine.d[f];
	}
	drop_records(all, &mine);
	return 0;
}

/* FNV-1a over a run of bytes, continued from h */
static unsigned long long hist_hash(unsigned long long h, const void * p, size_t n)
{
	const unsigned char * b = (const unsigned char *)p;
	size_t i;
	for(i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ULL; }
	return h;
}

int pft_solver_hist(int nv, const int * vops, const double * vargs, int nm, const int * mops, const double * margs,
                    int nbins, const double * edges, pft_hist_head * global, long long * global_counts,
                    pft_hist_head * local, long long * local_counts, pft_hist_head * plane_heads,
                    long long * plane_counts)
{
	/* f13: the histogram of the device-resident x, under pft_solver_diag's rules.  Every rank checks
	   the edges and compiles both programs first; the outcome (compile_rank; bad edges are -2 as a
	   bad program is) and a 64-bit hash of nbins, the edges and both programs travel in one
	   allgather, so that ranks that were given different histograms all answer -2 before any device
	   work.  Then each rank counts its slab and the used part of its message travels
	   (gather_records); the records are merged in rank order */
	struct hist_first { long long code; unsigned long long hash; };
	struct hist_msg { long long status; pft_hist_head h; long long counts[PFT_HIST_MAX_BINS]; } mine;
	const struct hist_msg * m;
	char * all;
	struct hist_first first, firsts[PFT_DIAG_MAX_RANKS];
	pft_ic_prog pv, pm;
	pft_grid g;
	pft_comm * c = comm();
	const int nprocs = pft_comm_size(c);
	const int masked = mops || margs || nm;
	int rc, r;
	size_t used;
	if(!global || !global_counts) return -2;
	if((rc = resident_state(1))) return rc;
	if(nprocs > PFT_DIAG_MAX_RANKS) return -2;
	memset(&pv, 0, sizeof pv);
	memset(&pm, 0, sizeof pm);
	first.hash = 0xcbf29ce484222325ULL;
	if(nv < 1 || nv > PFT_FORMULA_MAX_ENTRIES || !vops || !vargs || pft_hist_check(nbins, edges)
	   || (masked && (nm < 1 || !mops || !margs || nv + nm > PFT_FORMULA_MAX_ENTRIES)) || pft_model_get_grid(&g)) rc = -2;
	if(!rc) {
		first.hash = hist_hash(first.hash, &nbins, sizeof nbins);
		first.hash = hist_hash(first.hash, edges, sizeof(double) * ((size_t)nbins + 1));
		first.hash = hist_hash(first.hash, &nv, sizeof nv);
		first.hash = hist_hash(first.hash, vops, sizeof(int) * (size_t)nv);
		first.hash = hist_hash(first.hash, vargs, sizeof(double) * (size_t)nv);
		first.hash = hist_hash(first.hash, &nm, sizeof nm);
		if(masked) {
			first.hash = hist_hash(first.hash, mops, sizeof(int) * (size_t)nm);
			first.hash = hist_hash(first.hash, margs, sizeof(double) * (size_t)nm);
		}
		rc = pft_formula_compile(&g, nv, vops, vargs, &pv);
		if(!rc && masked) rc = pft_formula_compile(&g, nm, mops, margs, &pm);
	}
	if(nprocs > 1) {
		int crc;
		long long v = 0;
		first.code = compile_rank(rc);
		crc = pft_comm_allgather(c, &first, (int)sizeof first, firsts);
		if(crc) {
			pft_ic_prog_free(&pv);
			pft_ic_prog_free(&pm);
			R.last_status = crc;
			return PFT_SOLVE_DEVICE_ERROR;
		}
		for(r = 0; r < nprocs; r++) if(firsts[r].code > v) v = firsts[r].code;
		/* (ranks that all compiled: the same histogram on every one of them, or -2) */
		for(r = 1; r < nprocs && !v; r++) if(firsts[r].hash != firsts[0].hash) v = 2;
		rc = compile_code(v);
	}
	if(rc) {
		pft_ic_prog_free(&pv);
		pft_ic_prog_free(&pm);
		return rc;
	}
	memset(&mine, 0, sizeof mine);
	rc = pft_slab_hist(R.slab, PFT_BUF_X, &pv, masked ? &pm : NULL, nbins, edges, &mine.h, mine.counts, plane_heads,
	                   plane_counts);
	pft_ic_prog_free(&pv);
	pft_ic_prog_free(&pm);
	used = offsetof(struct hist_msg, counts) + (size_t)nbins * sizeof(long long);
	if((rc = gather_records(rc, &mine, used, &all))) return rc;
	m = (const struct hist_msg *)all;
	*global = m->h;
	memcpy(global_counts, m->counts, sizeof(long long) * (size_t)nbins);
	for(r = 1; r < nprocs; r++) {
		m = (const struct hist_msg *)(all + (size_t)r*used);
		pft_hist_combine(nbins, global, global_counts, &m->h, m->counts);
	}
	if(local) *local = mine.h;
	if(local_counts) memcpy(local_counts, mine.counts, sizeof(long long) * (size_t)nbins);
	drop_records(all, &mine);
	return 0;
}

int pft_solver_map(int nv, const int * vops, const double * vargs, int nm, const int * mops, const double * margs,
                   int axis, pft_map_px * global, pft_map_px * local)
{
	/* f15: the map of the device-resident x, under pft_solver_hist's rules.  Every rank compiles both
	   programs first; the outcome, a 64-bit hash of the axis, of whether a global map is wanted and
	   of both programs, and the slab's rows travel in one allgather, so that ranks that were given
	   different maps all answer -2 before any device work.  Then each rank reduces its slab.  With
	   `global` its share travels with its status (gather_records): for axis 0 its partial map, merged
	   in rank order; for axes 1 and 2 its rows, every rank sending as many as the tallest slab has
	   (the rest neutral), put at the slab's first row.  Without `global` only the status travels. */
	struct map_first { long long code; unsigned long long hash; long long n3, first_row; };
	char * all, * msg = NULL;
	long long status_only = 0;
	struct map_first first, firsts[PFT_DIAG_MAX_RANKS];
	pft_ic_prog pv, pm;
	pft_grid g;
	pft_comm * c = comm();
	const int nprocs = pft_comm_size(c);
	const int masked = mops || margs || nm;
	const int want_global = global != NULL;
	int rc, r, rows = 0, cols = 0;
	long q, n = 0, send = 0, max_n3 = 0;
	size_t used = sizeof status_only;
	if(!local) return -2;
	if((rc = resident_state(1))) return rc;
	if(nprocs > PFT_DIAG_MAX_RANKS) return -2;
	memset(&pv, 0, sizeof pv);
	memset(&pm, 0, sizeof pm);
	memset(&first, 0, sizeof first);
	first.hash = 0xcbf29ce484222325ULL;
	if(nv < 1 || nv > PFT_FORMULA_MAX_ENTRIES || !vops || !vargs || axis < 0 || axis > 2
	   || (masked && (nm < 1 || !mops || !margs || nv + nm > PFT_FORMULA_MAX_ENTRIES)) || pft_model_get_grid(&g)
	   || pft_map_dims(&g, axis, &rows, &cols)) rc = -2;
	if(!rc) {
		first.hash = hist_hash(first.hash, &axis, sizeof axis);
		first.hash = hist_hash(first.hash, &want_global, sizeof want_global);
		first.hash = hist_hash(first.hash, &nv, sizeof nv);
		first.hash = hist_hash(first.hash, vops, sizeof(int) * (size_t)nv);
		first.hash = hist_hash(first.hash, vargs, sizeof(double) * (size_t)nv);
		first.hash = hist_hash(first.hash, &nm, sizeof nm);
		if(masked) {
			first.hash = hist_hash(first.hash, mops, sizeof(int) * (size_t)nm);
			first.hash = hist_hash(first.hash, margs, sizeof(double) * (size_t)nm);
		}
		first.n3 = g.n3;
		first.first_row = g.first_row;
		rc = pft_formula_compile(&g, nv, vops, vargs, &pv);
		if(!rc && masked) rc = pft_formula_compile(&g, nm, mops, margs, &pm);
	}
	if(nprocs > 1) {
		int crc;
		long long v = 0;
		first.code = compile_rank(rc);
		crc = pft_comm_allgather(c, &first, (int)sizeof first, firsts);
		if(crc) {
			pft_ic_prog_free(&pv);
			pft_ic_prog_free(&pm);
			R.last_status = crc;
			return PFT_SOLVE_DEVICE_ERROR;
		}
		for(r = 0; r < nprocs; r++) if(firsts[r].code > v) v = firsts[r].code;
		/* (ranks that all compiled: the same map on every one of them, or -2) */
		for(r = 1; r < nprocs && !v; r++) if(firsts[r].hash != firsts[0].hash) v = 2;
		rc = compile_code(v);
	}
	if(rc) {
		pft_ic_prog_free(&pv);
		pft_ic_prog_free(&pm);
		return rc;
	}
	n = (long)rows * cols;
	if(nprocs > 1 && want_global) {
		/* what every rank sends: its partial map (axis 0), or as many rows as the tallest slab has */
		long long bad;
		for(r = 0; r < nprocs; r++) if(firsts[r].n3 > max_n3) max_n3 = (long)firsts[r].n3;
		send = axis == 0 ? n : max_n3 * cols;
		used = sizeof status_only + sizeof(pft_map_px) * (size_t)send;
		msg = (char *)malloc(used);
		bad = !msg;
		if((rc = pft_comm_allreduce_max_i64(c, &bad)) || bad) {
			free(msg);
			pft_ic_prog_free(&pv);
			pft_ic_prog_free(&pm);
			if(rc) R.last_status = rc;
			return rc ? PFT_SOLVE_DEVICE_ERROR : -1;
		}
	}
	rc = pft_slab_map(R.slab, PFT_BUF_X, &pv, masked ? &pm : NULL, axis, local);
	pft_ic_prog_free(&pv);
	pft_ic_prog_free(&pm);
	if(!rc && axis == 0 && g.first_row) {
		/* the slab counts its own planes from 0 */
		for(q = 0; q < n; q++) {
			if(local[q].first >= 0) local[q].first += g.first_row;
			if(local[q].last >= 0) local[q].last += g.first_row;
		}
	}
	if(msg) {
		pft_map_px * rec = (pft_map_px *)(msg + sizeof status_only);
		if(!rc) memcpy(rec, local, sizeof(pft_map_px) * (size_t)n);
		for(q = rc ? 0 : n; q < send; q++) pft_map_init(&rec[q]);
	}
	rc = gather_records(rc, msg ? (void *)msg : (void *)&status_only, used, &all);
	if(rc) {
		free(msg);
		return rc;
	}
	if(global && nprocs == 1) memcpy(global, local, sizeof(pft_map_px) * (size_t)n);
	else if(global) {
		const long total = axis == 0 ? n : (long)g.total_n3 * cols;
		for(q = 0; q < total; q++) pft_map_init(&global[q]);
		for(r = 0; r < nprocs; r++) {
			const pft_map_px * rec = (const pft_map_px *)(all + (size_t)r*used + sizeof status_only);
			if(axis == 0) pft_map_combine(n, global, rec);
			else memcpy(global + firsts[r].first_row * cols, rec, sizeof(pft_map_px) * (size_t)(firsts[r].n3 * cols));
		}
	}
	drop_records(all, msg ? (void *)msg : (void *)&status_only);
	free(msg);
	return 0;
}

/* the common end of the device IC paths: every rank's outcome agreed (a rank that failed locally
   still takes part, so that no other rank is left inside a collective: every rank returns the same,
   most negative, code), then the ghost planes exchanged as at an upload and gl_keep agreed */
static int ic_device_finish(int ret, int unclean)
{
	pft_comm * c = comm();
	const long long FAILED = 1LL << 40;
	long long u = ret ? FAILED - ret : unclean;
	int rc;
	if(pft_comm_size(c) > 1 && (rc = pft_comm_allreduce_max_i64(c, &u))) {
		R.last_status = rc;
		return PFT_SOLVE_DEVICE_ERROR;
	}
	if(u >= FAILED) return (int)(FAILED - u);
	if(pft_comm_size(c) > 1) {
		if((rc = pft_comm_halo(c, PFT_BUF_X, 0, 3)) || (rc = pft_comm_halo(c, PFT_BUF_XN, 0, 3))) {
			R.last_status = rc;
			return PFT_SOLVE_DEVICE_ERROR;
		}
	}
	pft_slab_set_gl_keep(R.slab, !u);
	R.device_valid = 1;
	R.k1_keep = 0;
	return 0;
}

int pft_solver_ic_default_device(int with_beads)
{
	/* f1: the default Params' IC (and the glass beads) computed on the device into X and XN, bit
	   for bit what pft_model_ic_default + PrecalculateData give on the host; the next
	   pft_solve_ex(..., PFT_SOLVE_REUSE_DEVICE) starts from it.  Collective with nprocs > 1 (the
	   ghost planes are exchanged, as at an upload, and the ranks agree on gl_keep). */
	pft_ic_tables tb;
	double * store = NULL;
	int * istore = NULL, unclean = 0, rc, ret = 0;
	if(R.max_n == 0) return -3;
	if((rc = ensure_slab())) { R.last_status = rc; ret = PFT_SOLVE_DEVICE_ERROR; }
	else if((rc = pft_model_ic_tables(&tb, with_beads, &store, &istore))) ret = rc;
	else {
		rc = pft_slab_ic_default(R.slab, &tb, &unclean);
		if(rc) { R.last_status = rc; ret = PFT_SOLVE_DEVICE_ERROR; }
	}
	free(store);
	free(istore);
	return ic_device_finish(ret, unclean);
}

int pft_solver_ic_formulas_device(int nprog, const int * qs, const int * lens, const int * ops,
                                  const double * args, int with_beads)
{
	pft_grid g;
	pft_ic_tables tb;
	pft_ic_prog * pr;
	double * store = NULL;
	int * istore = NULL, unclean = 0, rc = 0, crc, ret = 0, p, off = 0, ok = 1;
	if(R.max_n == 0) return -3;
	if(nprog < 1 || !qs || !lens || !ops || !args || pft_model_get_grid(&g)) return -2;
	pr = (pft_ic_prog*)calloc(nprog, sizeof(pft_ic_prog));
	if(!pr) return -1;
	/* compile every program first: the device is not touched unless all of them compile.  The
	   outcome is agreed across ranks before anything collective: 1 (stays on the host) and -2 (bad
	   program) are the same on every rank, but -1 (out of memory in the compiler's tables) is local,
	   and a rank returning early would leave the others in ensure_slab's attach rounds or the
	   allreduce of ic_device_finish until the transport's timeout.  Every rank returns the same code:
	   -1 over -2 over 1. */
	for(p = 0; p < nprog && ok; p++) {
		if(qs[p] < 0 || qs[p] > 2 || lens[p] < 1) { ok = 0; rc = -2; break; }
		rc = pft_ic_compile(&g, lens[p], ops + off, args + off, &pr[p]);
		off += lens[p];
		if(rc) ok = 0;
	}
	if((crc = compile_agree(&rc))) {
		R.last_status = crc;
		rc = PFT_SOLVE_DEVICE_ERROR;
	}
	ok = rc == 0;
	if(!ok) {
		for(p = 0; p < nprog; p++) pft_ic_prog_free(&pr[p]);
		free(pr);
		return rc;
	}
	if((rc = ensure_slab())) { R.last_status = rc; ret = PFT_SOLVE_DEVICE_ERROR; }
	for(p = 0; p < nprog && !ret; p++)
		if((rc = pft_slab_ic_program(R.slab, qs[p], &pr[p], p == 0))) { R.last_status = rc; ret = PFT_SOLVE_DEVICE_ERROR; }
	for(p = 0; p < nprog; p++) pft_ic_prog_free(&pr[p]);
	free(pr);
	/* the beads over gl (PrecalculateData, equation.c:459-530), or only the gl scan without them */
	if(!ret && (rc = pft_model_ic_tables(&tb, with_beads, &store, &istore))) ret = rc;
	else if(!ret && (rc = pft_slab_ic_beads(R.slab, &tb, &unclean))) { R.last_status = rc; ret = PFT_SOLVE_DEVICE_ERROR; }
	free(store);
	free(istore);
	return ic_device_finish(ret, unclean);
}

int pft_solver_ic_beads_device(void)
{
	/* the glass beads over the gl already in X and XN (a state read by pft_solver_snapshot_read:
	   the reference overlays them on a file's state too, equation.c:507-530 -- a max, so idempotent
	   on the case's own file), ended as every device IC */
	pft_ic_tables tb;
	double * store = NULL;
	int * istore = NULL, unclean = 0, rc, ret = 0;
	if(R.max_n == 0 || !R.slab || !R.device_valid) return -3;
	if((rc = pft_model_ic_tables(&tb, 1, &store, &istore))) ret = rc;
	else if((rc = pft_slab_ic_beads(R.slab, &tb, &unclean))) { R.last_status = rc; ret = PFT_SOLVE_DEVICE_ERROR; }
	free(store);
	free(istore);
	return ic_device_finish(ret, unclean);
}

/* ---------------------------------------------------------------------------------------- */
/* f7: snapshots from and into the resident state */

/* the host link of a device snapshot: kept after the measurement of DESIGN.md section 7 f7; env
   PFT_SNAP_LINK=0/1 (direct / staged) overrides it for that A/B */
static int snap_link(int flags)
{
	const char * e = getenv("PFT_SNAP_LINK");
	if(flags & PFT_SNAP_STAGED) return PFT_SNAP_LINK_STAGED;
	if(flags & PFT_SNAP_DIRECT) return PFT_SNAP_LINK_DIRECT;
	if(e && (e[0] == '0' || e[0] == '1') && !e[1]) return e[0] - '0';
	return PFT_SNAP_LINK_DEFAULT;
}

/* the ranks agree a status: every rank returns the most negative code (0: all well) */
static int snap_agree(int rc)
{
	pft_comm * c = comm();
	long long v = -(long long)rc;
	int crc;
	if(pft_comm_size(c) == 1) return rc;
	if((crc = pft_comm_allreduce_max_i64(c, &v))) { R.last_status = crc; return PFT_SOLVE_DEVICE_ERROR; }
	return (int)-v;
}

int pft_solver_snapshot_write(const char * path, const double * param, const pft_snapshot_info * info, int flags)
{
	const int version = (flags >> 8) & 3;
	pft_snapshot_ranges r;
	void * image = NULL;
	int rc = 0;
	if(!path || !param || !info || version > 2) return -2;
	/* the validity rules of pft_solver_diag: never a stale file */
	if((rc = resident_state(1))) return rc;
	/* rank 0 writes the header; the agreed status is also the barrier before the other ranks open
	   the file */
	if(R.slab_grid.rank == 0) rc = pft_snapshot_create(path, &R.slab_grid, param, info, version);
	if((rc = snap_agree(rc))) return rc;
	rc = pft_snapshot_slab_ranges(path, &R.slab_grid, &r);
	/* the image leaves the device: when this returns, the next solve may overwrite X */
	if(!rc && (rc = pft_slab_snapshot_export(R.slab, PFT_BUF_X, snap_link(flags), &image))) {
		R.last_status = rc;
		rc = PFT_SOLVE_DEVICE_ERROR;
	}
	if(!rc) rc = pft_snapshot_write_image_async(path, &r, image);
	if(!rc && !(flags & PFT_SNAP_ASYNC)) rc = pft_snapshot_writer_wait();
	return snap_agree(rc);
}

/* f11: the region with its k triple made slab-local (what the slab's entries take) */
static int region_of_slab(const pft_region * region, pft_region * loc, int * kfirst)
{
	int kcount, klocal, rc;
	if((rc = pft_region_local(&R.slab_grid, region, kfirst, &kcount, &klocal))) return rc;
	*loc = *region;
	loc->start[2] = klocal;
	loc->count[2] = kcount;
	return 0;
}

int pft_solver_snapshot_region_write(const char * path, const double * param, const pft_snapshot_info * info,
                                     const pft_region * region, int flags)
{
	const int version = (flags >> 8) & 3;
	pft_snapshot_ranges r;
	pft_region loc;
	void * image = NULL;
	int rc = 0, kfirst;
	if(!path || !param || !info || !region || version > 2) return -2;
	if((rc = resident_state(1))) return rc;
	/* the region is judged against the whole grid, which every rank holds: the same answer everywhere */
	if(pft_region_check(&R.slab_grid, region)) return -2;
	if(R.slab_grid.rank == 0) rc = pft_snapshot_create_region(path, &R.slab_grid, region, param, info, version);
	if((rc = snap_agree(rc))) return rc;
	rc = pft_snapshot_region_ranges(path, &R.slab_grid, region, &r);
	if(!rc) rc = region_of_slab(region, &loc, &kfirst);
	if(!rc && loc.count[2] > 0) {
		if((rc = pft_slab_region_export(R.slab, PFT_BUF_X, &loc, snap_link(flags), &image))) {
			R.last_status = rc;
			rc = PFT_SOLVE_DEVICE_ERROR;
		}
		if(!rc) rc = pft_snapshot_write_image_async(path, &r, image);
	}
	if(!rc && !(flags & PFT_SNAP_ASYNC)) rc = pft_snapshot_writer_wait();
	return snap_agree(rc);
}

int pft_solver_region(const pft_region * region, double * out_native)
{
	pft_region loc;
	void * image = NULL;
	int rc, kfirst;
	size_t n, w;
	if(!region) return -2;
	if((rc = resident_state(0))) return rc;
	if((rc = region_of_slab(region, &loc, &kfirst))) return rc;
	n = 3 * (size_t)loc.count[0] * (size_t)loc.count[1] * (size_t)loc.count[2];
	if(n == 0) return 0;
	if(!out_native) return -2;
	if((rc = pft_slab_region_export(R.slab, PFT_BUF_X, &loc, snap_link(0), &image))) {
		R.last_status = rc;
		return PFT_SOLVE_DEVICE_ERROR;
	}
	for(w = 0; w < n; w++) {
		unsigned long long v;
		memcpy(&v, (const char *)image + 8 * w, 8);
		v = __builtin_bswap64(v);
		memcpy(out_native + w, &v, 8);
	}
	return 0;
}

int pft_solver_snapshot_wait(void)
{
	return snap_agree(pft_snapshot_writer_wait());
}

int pft_solver_snapshot_read(const char * path)
{
	pft_grid g;
	pft_snapshot_ranges r;
	void * image = NULL;
	int rc, ret = 0, unclean = 0;
	if(!path) return -2;
	if(R.max_n == 0) return -3;
	if(pft_model_get_grid(&g)) return -2;
	/* the header, and with it a dimension mismatch (-4, the same on every rank), before any device
	   work; every rank returns the agreed code */
	rc = pft_snapshot_slab_ranges(path, &g, &r);
	if((rc = snap_agree(rc))) return rc;
	if((rc = ensure_slab())) { R.last_status = rc; ret = PFT_SOLVE_DEVICE_ERROR; }
	else if((rc = pft_slab_image(R.slab, &image, NULL))) { R.last_status = rc; ret = PFT_SOLVE_DEVICE_ERROR; }
	else {
		/* each rank reads only its own planes, into the slab's pinned image, which the import kernel
		   reads in place */
		void * dev = NULL;
		pft_snapshot_writer_release(image);
		pft_slab_image(R.slab, NULL, &dev);
		if((rc = pft_snapshot_read_image(path, &r, image))) ret = rc;
		else if((rc = pft_slab_import_be(R.slab, dev, &unclean))) { R.last_status = rc; ret = PFT_SOLVE_DEVICE_ERROR; }
	}
	return ic_device_finish(ret, unclean);
}

int pft_solver_eval_rhs(FLOAT t, const FLOAT * w, FLOAT * dw)
{
	/* f(t, w, dw) on host arrays: stage w into A0, exchange its boundary planes, K into K1 */
	pft_comm * c = comm();
	int rc;
	R.k1_keep = 0;                       /* K1's buffer receives this K */
	if(R.fail_rhs_after > 0 && ++R.rhs_calls >= R.fail_rhs_after) {
		R.fail_rhs_after = 0;
		rc = -1000 - 999;                    /* as a hipError_t the runtime reports for a fault */
	} else if(!(rc = ensure_slab()) && !(rc = pft_slab_upload_host(R.slab, PFT_BUF_A0, w)) &&
	   !(pft_comm_size(c) > 1 && (rc = pft_comm_halo(c, PFT_BUF_A0, 0, 3))) &&
	   !(rc = pft_slab_rhs(R.slab, PFT_BUF_A0, PFT_BUF_K1, t)))
		rc = pft_slab_download_host(R.slab, PFT_BUF_K1, dw);
	if(rc) {
		R.last_status = rc;
		R.rhs_failed = 1;
	}
	return rc;
}

/* ---------------------------------------------------------------------------------------- */
/* host-staged path: any right-hand side, combines on the GPU over the chunk table */

static int alloc_staged(void)
{
	int rc;
	if(R.d_cap >= R.max_n) return 0;
	free_staged();
	if((rc = pft_flat_alloc(&R.d_x, R.max_n)) || (rc = pft_flat_alloc(&R.d_k1, R.max_n)) ||
	   (rc = pft_flat_alloc(&R.d_k3, R.max_n)) || (rc = pft_flat_alloc(&R.d_k4, R.max_n)) ||
	   (rc = pft_flat_alloc(&R.d_k5, R.max_n)) || (rc = pft_flat_alloc(&R.d_aux, R.max_n)) ||
	   (rc = pft_flat_alloc(&R.d_eps, 2))) return rc;
	R.d_cap = R.max_n;
	R.h_k = (double*)calloc(R.max_n, sizeof(double));
	R.h_aux = (double*)calloc(R.max_n, sizeof(double));
	if(!R.h_k || !R.h_aux) return -1;
	return 0;
}

static int ensure_staged(const RK_MEM_DIST * n)
{
	int rc;
	if((rc = alloc_staged())) return rc;
	if(R.d_nch < n->n_chunks) {
		pft_dev_free(R.d_cs); pft_dev_free(R.d_cz); pft_flat_free(R.d_cm);
		if((rc = pft_dev_alloc((void**)&R.d_cs, sizeof(int)*n->n_chunks)) ||
		   (rc = pft_dev_alloc((void**)&R.d_cz, sizeof(int)*n->n_chunks)) ||
		   (rc = pft_flat_alloc(&R.d_cm, n->n_chunks))) return rc;
		R.d_nch = n->n_chunks;
	}
	if((rc = pft_h2d(R.d_cs, n->chunk_start, sizeof(int)*n->n_chunks, NULL))) return rc;
	if((rc = pft_h2d(R.d_cz, n->chunk_size, sizeof(int)*n->n_chunks, NULL))) return rc;
	if(n->chunk_eps_mult) {
		if((rc = pft_flat_h2d(R.d_cm, n->chunk_eps_mult, n->n_chunks, NULL))) return rc;
	} else {
		double * ones = (double*)malloc(sizeof(double)*n->n_chunks);
		int i;
		for(i=0;i<n->n_chunks;i++) ones[i] = 1.0;
		rc = pft_flat_h2d(R.d_cm, ones, n->n_chunks, NULL);
		free(ones);
		if(rc) return rc;
	}
	return pft_stream_sync(NULL);
}

static int staged_rhs(RK_RightHandSide f, double t, const double * d_in, double * host_in, double * d_out)
{
	int rc;
	if(d_in) {
		if((rc = pft_flat_d2h(host_in, d_in, R.max_n, NULL)) || (rc = pft_stream_sync(NULL))) return rc;
	}
	R.rhs_failed = 0;
	f(t, host_in, R.h_k);
	if(R.rhs_failed) {
		/* libpft's own f failed on the device and left NaN in h_k: never let that pass as a step
		   (the reference driver leaves NaN handling off, intertrack.c:2193) */
		R.rhs_failed = 0;
		return R.last_status <= -1000 ? R.last_status : -1;
	}
	if((rc = pft_flat_h2d(d_out, R.h_k, R.max_n, NULL))) return rc;
	return 0;
}

static int run_staged(RK_MPI_S_SOLUTION * system, RK_RightHandSide f, solve_bcast * B, long max_steps_total, int flags)
{
	R.k1_keep = 0;                       /* this path computes K1 in the slab's buffers */
	pft_comm * c = comm();
	const int nprocs = pft_comm_size(c);
	RK_MEM_DIST * n = system->n;
	double * x = system->x;
	step_loop L = {system, B, max_steps_total};
	double eps;
	int rc, nch = n->n_chunks;
	double zero2[2] = {0.0, 0.0};
	(void)flags;

	if((rc = ensure_staged(n))) return rc;
	if((rc = pft_flat_h2d(R.d_x, x, R.max_n, NULL))) return rc;
	R.stats.path = 2;

	while(1) {
		const double t = B->a.t, h = B->a.h;
		double * const kbuf[6] = {NULL, R.d_k1, R.d_k3, R.d_k3, R.d_k4, R.d_k5};   /* K2 in K3's buffer */
		long long bits[2];
		int st;
		for(st = 1; st <= 5; st++) {
			/* K = f(ts, stage input), then the stage's combine into aux, stage 5's into the error norm (:373-453, 507-524) */
			const pft_stage_scalars s = pft_stepctl_stage(st, t, h);
			if((rc = staged_rhs(f, s.ts, st == 1 ? NULL : R.d_aux, st == 1 ? x : R.h_aux, kbuf[st]))) return rc;
			if(st == 5 && (rc = pft_flat_h2d(R.d_eps, zero2, 2, NULL))) return rc;
			if((rc = pft_flat_combine(st, nch, R.d_cs, R.d_cz, R.d_cm, s.coef, h, R.d_x, R.d_k1, R.d_k3, R.d_k3,
			                          R.d_k4, R.d_k5, R.d_aux, R.d_eps, NULL))) return rc;
		}
		if((rc = pft_flat_d2h((double*)bits, R.d_eps, 2, NULL)) || (rc = pft_stream_sync(NULL))) return rc;
		if(nprocs > 1) {
			if((rc = pft_comm_allreduce_max_i64(c, &bits[0]))) return rc;                      /* :572 */
			bits[1] &= 0xffffffffLL;
			if((rc = pft_comm_allreduce_max_i64(c, &bits[1]))) return rc;
		}
		memcpy(&eps, &bits[0], sizeof(double));
		if(step_judge(&L, eps, (bits[1] & 0xffffffffLL) != 0)) break;
		if(pft_stepctl_accepted(L.command)) {
			int ch;
			if((rc = pft_flat_combine(6, nch, R.d_cs, R.d_cz, R.d_cm, pft_stepctl_stage(5, t, h).coef, h, R.d_x, R.d_k1, R.d_k3,
			                          R.d_k3, R.d_k4, R.d_k5, R.d_x, R.d_eps, NULL))) return rc;    /* :657-668 */
			/* the right-hand side of the next step reads the host x: only the chunks (the
			   unknowns) come back, the ghost values the last f(t, x) wrote stay (the
			   reference updates x in place, hybrid2.c:657-668) */
			if((rc = pft_flat_d2h(R.h_aux, R.d_x, R.max_n, NULL)) || (rc = pft_stream_sync(NULL))) return rc;
			for(ch = 0; ch < nch; ch++)
				memcpy(x + n->chunk_start[ch], R.h_aux + n->chunk_start[ch], sizeof(double)*n->chunk_size[ch]);
			if((rc = step_accepted(&L, 0)) < 0) return rc;
			if(rc) break;
			if(system->DDLBF_Rearrange != NULL) {                                              /* :726-729 */
				n = system->n = system->DDLBF_Rearrange(n);
				nch = n->n_chunks;
				if((rc = ensure_staged(n))) return rc;
			}
			f = system->meta_f();                                                              /* :732 */
		}
		if(step_next(&L)) break;
	}
	system->t = B->a.t;                                                                           /* :768 */
	R.stats.steps_total = L.attempted;
	R.stats.kernel_launches = 6*L.attempted;
	return L.ret;
}

/* ---------------------------------------------------------------------------------------- */
/* solve, hybrid2.c:215-337 prologue */

int pft_solve_ex(FLOAT final_time, RK_MPI_S_SOLUTION * system, long max_steps_total, int flags)
{
	pft_comm * c = comm();
	const int rank = pft_comm_rank(c);
	int error_code = 0, crc;
	long long neg;
	RK_RightHandSide f = NULL;
	solve_bcast B;
	RK_MEM_DIST * n;

	if(system == NULL) return -2;                                               /* :249 */
	n = system->n;
	if(system->meta_f != NULL) f = system->meta_f();                            /* :268 */
	if(n == NULL || n->n_chunks <= 0) error_code = -5;                          /* :276-280 */
	else if(n->chunk_start[n->n_chunks-1] + n->chunk_size[n->n_chunks-1] > R.max_n) error_code = -5;
	if(R.max_n == 0) error_code = -3;                                           /* :282 */
	if(system->x == NULL || system->meta_f == NULL) error_code = -2;            /* :284 */
	if(rank == R.master && system->delta <= 0) error_code = -2;                 /* :286 */
	neg = -error_code;                                                          /* :294 Allreduce(MIN) */
	/* a failed collective (a lost peer, an aborted communicator) is a device error on every rank
	   that sees it; the bounded waits inside make sure each one returns */
	if((crc = pft_comm_allreduce_max_i64(c, &neg))) { R.last_status = crc; return PFT_SOLVE_DEVICE_ERROR; }
	if(error_code) return error_code;                                           /* :295 */
	if(neg > 0) return -6;                                                      /* :299 */

	R.last_nan = 0;                                                             /* :316 */
	B.k.final_time = final_time; B.k.delta = system->delta; B.k.h_min = system->h_min;
	B.k.delta_local = system->delta_mode == DELTA_LOCAL; B.k.handle_nan = R.handle_nan;
	B.a.t = system->t; B.a.h = system->h; B.a.command = 0;
	B.any_cb = system->Service_Callback != NULL;
	if(rank == R.master) {                                                      /* :319-325 */
		if((final_time > B.a.t && B.a.h < 0) || (final_time < B.a.t && B.a.h > 0)) B.a.h *= -1;
		if(B.a.h == 0 || fabs(final_time - B.a.t) <= fabs(B.a.h)) {
			B.a.h = final_time - B.a.t;
			B.a.command |= RKA_CMD_FINISHED;
		}
	}
	if(pft_comm_size(c) > 1) {                                                  /* :328-336 */
		long long cmd = B.a.command;
		if((crc = pft_comm_bcast(c, &B, sizeof(B), R.master)) || (crc = pft_comm_allreduce_max_i64(c, &cmd))) {
			R.last_status = crc;
			return PFT_SOLVE_DEVICE_ERROR;
		}
		B.a.command = (int)cmd;
	}
	R.stats.nprocs = pft_comm_size(c);
	R.stats.rank = rank;

	{
		int rc;
		double em[3];
		if(pft_model_is_device_rhs(f) && system->DDLBF_Rearrange == NULL && canonical_chunks(n, em))
			rc = run_fused(system, f, &B, max_steps_total, flags, em);
		else
			rc = run_staged(system, f, &B, max_steps_total, flags);
		/* a HIP or RCCL failure (out of device memory, a lost peer, ...) is reported as
		   PFT_SOLVE_DEVICE_ERROR; the raw status stays in pft_solver_last_status() and the HIP
		   text in pft_hip_last_error() */
		if(rc <= -1000 || rc == -1) {
			R.last_status = rc;
			R.device_valid = 0;
			return PFT_SOLVE_DEVICE_ERROR;
		}
		return rc;
	}
}

int RK_MPI_SA_solve(FLOAT final_time, RK_MPI_S_SOLUTION * system)
{
	return pft_solve_ex(final_time, system, 0, 0);
}
