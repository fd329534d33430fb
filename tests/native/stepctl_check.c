/* stepctl_check.c -- the step controller of porousfreezethaw_amd/csrc/pft_stepctl.h on the CPU, over
   that header alone (tests/test_stepctl.py; `make -C porousfreezethaw_amd stepctl-selftest`).

   Holds a verbatim copy of the controller as rk_solver.c's run_fused wrote it inline before the
   header existed (without the callbacks), and of the arithmetic of the device's gate_decide of that
   time with the C library's pow in place of pow02_rn, and checks bit for bit:
     1. the header's judgement and advance against the copied loop body over a fixed-seed sweep:
        the command, t, h, new_h, the stored system->h and the -4 exit;
     2. the gate invariant: wherever the host accepts and goes on, the gate form yields exactly the
        host's next (t, h), everywhere else a skip -- and the header gives the copied gate's answer;
     3. multi-step chains with scripted error norms to FINISHED at exactly final_time;
     4. the stage scalars against the literal expressions.
   Prints "<sweep cases> <chain steps> <scalar cases>"; exit status 1 on the first mismatch. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../porousfreezethaw_amd/csrc/pft_stepctl.h"

/* (the header brings RKA_CMD_* and DELTA_LOCAL / DELTA_GLOBAL of include/RK_MPI_SAsolver.h) */

/* ---- the copies ----------------------------------------------------------------------------- */

typedef struct {
	double final_time, delta, h_min;
	int delta_mode, handle_nan;
} old_consts;

typedef struct {
	double t, h, new_h;        /* the loop's variables */
	int command;
	int judged;                /* command as judged, before the branches consumed it */
	double sys_t, sys_h;       /* system->t, system->h (NaN pattern below: never stored) */
	int ret, last_nan, acc, ended;
	long steps, attempted;
} old_loop;

/* one pass of the loop body from the error norm on; ended: the loop broke */
static void old_body(const old_consts * B, old_loop * o, double eps, int nonfinite)
{
	const double final_time = B->final_time, delta = B->delta, h_min = B->h_min;
	double t = o->t, h = o->h, new_h;
	int command = o->command;
	const double h3 = h/3.0;
	o->acc = 0;
	o->attempted++;
	do {
		if(B->handle_nan && nonfinite) {                                         /* :493-503 */
			command |= RKA_CMD_NAN;
			if(h/(final_time-t) < 1e-11) command |= RKA_CMD_h_TOO_SMALL;
		}
		if(B->delta_mode == DELTA_LOCAL) eps *= fabs(h3);                        /* :578 */
		new_h = ((eps > 0.0) ? pow((delta/eps), 0.2)*0.8 : 2.0) * h;            /* :580 */
		if(eps < delta || fabs(h) < h_min) {                                     /* :599-611 */
			command |= RKA_CMD_UPDATE;
			if(fabs(final_time-(t+h)) <= fabs(new_h)) command |= RKA_CMD_NEXTFINISH;
		}
		o->judged = command;
		o->new_h = new_h;

		if(command & RKA_CMD_NAN) {                                              /* :626-646 */
			o->last_nan = 1;
			if(command & RKA_CMD_h_TOO_SMALL) { o->sys_t = t; o->ret = -4; o->ended = 1; break; }
			h /= 10;
			command = 0;
		} else {
			if(command & RKA_CMD_UPDATE) {                                       /* :651-668 */
				t += h;
				o->acc = 1;
				o->steps++;
				if(command & RKA_CMD_FINISHED) { o->ended = 1; break; }          /* :695 */
			}
			if(command & RKA_CMD_NEXTFINISH) {                                   /* :743-761 */
				o->sys_h = new_h;
				h = final_time - t;
				command = RKA_CMD_FINISHED;
			} else {
				command = 0;
				h = new_h;
			}
		}
	} while(0);
	o->t = t; o->h = h; o->command = command;
}

/* gate_decide's arithmetic: 1 and the next (t, h), or 0: a skip */
static int old_gate(const old_consts * B, double t, double h, double eps, int nf, double * tn_out, double * hn_out)
{
	const double d_final = B->final_time, d_delta = B->delta, d_hmin = B->h_min;
	const int d_local = B->delta_mode == DELTA_LOCAL, d_nan = B->handle_nan;
	if (!(d_nan && nf)) {                                                    /* :493-503 */
		const double h3 = h / 3.0;
		if (d_local) eps *= fabs(h3);                                        /* :578 */
		const double new_h = ((eps > 0.0) ? pow((d_delta / eps), 0.2) * 0.8 : 2.0) * h;   /* :580 */
		if (eps < d_delta || fabs(h) < d_hmin) {                             /* :599-611 */
			const double tn = t + h;                                         /* :652 */
			const double hn = (fabs(d_final - tn) <= fabs(new_h)) ? d_final - tn : new_h;   /* :743-761 */
			*tn_out = tn;
			*hn_out = hn;
			return 1;
		}
	}
	return 0;
}

/* ---- helpers -------------------------------------------------------------------------------- */

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rng(void)
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return rng_state;
}
static double uni(double a, double b) { return a + (b - a) * ((rng() >> 11) * 0x1p-53); }
static double logu(double a, double b) { return exp(uni(log(a), log(b))); }

static int same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static void fail(const char * what, const old_consts * B, double t, double h, double eps, int nf, int cmd)
{
	printf("MISMATCH %s: final %a delta %a h_min %a mode %d nan %d | t %a h %a eps %a nf %d command %d\n", what,
	       B->final_time, B->delta, B->h_min, B->delta_mode, B->handle_nan, t, h, eps, nf, cmd);
	exit(1);
}

static pft_stepctl_consts consts_of(const old_consts * B)
{
	pft_stepctl_consts k;
	k.final_time = B->final_time; k.delta = B->delta; k.h_min = B->h_min;
	k.delta_local = B->delta_mode == DELTA_LOCAL; k.handle_nan = B->handle_nan;
	return k;
}

static const double NEVER = -12345.678;   /* system->t, system->h before the body stores them */

/* ---- 1, 2: one case ------------------------------------------------------------------------- */

static void one_case(const old_consts * B, double t, double h, double eps, int nf, int pending)
{
	const pft_stepctl_consts k = consts_of(B);
	const pft_step a = {t, h, pending};
	old_loop o;
	pft_step s;
	double tg = 0.0, hg = 0.0, new_h;
	int go, cmd, stores_h;
	memset(&o, 0, sizeof o);
	o.t = t; o.h = h; o.command = pending; o.sys_t = NEVER; o.sys_h = NEVER;
	old_body(B, &o, eps, nf);
	cmd = pft_stepctl_judge(k, a, eps, nf, &new_h);
	s = pft_stepctl_advance(k, a, cmd, new_h);
	stores_h = pft_stepctl_accepted(cmd) && (cmd & RKA_CMD_NEXTFINISH);

	if(cmd != o.judged) fail("judged command", B, t, h, eps, nf, pending);
	if(!same(new_h, o.new_h)) fail("new_h", B, t, h, eps, nf, pending);
	if(((cmd & RKA_CMD_NAN) != 0) != o.last_nan) fail("NaN flag", B, t, h, eps, nf, pending);
	if(((cmd & RKA_CMD_NAN) && (cmd & RKA_CMD_h_TOO_SMALL)) != (o.ret == -4)) fail("-4 exit", B, t, h, eps, nf, pending);
	if(pft_stepctl_accepted(cmd) != o.acc) fail("accept", B, t, h, eps, nf, pending);
	if(o.ret == -4) {
		/* the solve ends at the attempt's t: the advance of a NaN attempt leaves t alone */
		if(!same(o.sys_t, s.t)) fail("-4 exit's t", B, t, h, eps, nf, pending);
	} else if(o.ended) {
		/* accepted with FINISHED pending: the loop ends at the new t, before the tail */
		if(!(pending & RKA_CMD_FINISHED) || !same(s.t, o.t)) fail("FINISHED exit", B, t, h, eps, nf, pending);
	} else {
		if(!same(s.t, o.t)) fail("next t", B, t, h, eps, nf, pending);
		if(!same(s.h, o.h)) fail("next h", B, t, h, eps, nf, pending);
		if(s.command != o.command) fail("next command", B, t, h, eps, nf, pending);
		if(stores_h != !same(o.sys_h, NEVER) || (stores_h && !same(new_h, o.sys_h)))
			fail("stored system->h", B, t, h, eps, nf, pending);
	}

	/* the gate (never armed behind a step that ends the solve: no command pending) */
	if(!pending) {
		const int host_goes_on = o.acc && !o.ended;
		go = old_gate(B, t, h, eps, nf, &tg, &hg);
		if(go != host_goes_on) fail("gate go", B, t, h, eps, nf, pending);
		if(go && (!same(tg, o.t) || !same(hg, o.h))) fail("gate (t, h) against the host's", B, t, h, eps, nf, pending);
		if(pft_stepctl_accepted(cmd) != go || (go && (!same(s.t, tg) || !same(s.h, hg))))
			fail("header against the copied gate", B, t, h, eps, nf, pending);
	}
}

/* ---- 1, 2: the sweep ------------------------------------------------------------------------ */

#define N_SIGN 2
#define N_MODE 2
#define N_NAN 2
#define N_NF 2
#define N_PENDING 2
#define N_HKIND 8
#define N_EPS 12
#define N_REP 16

static long sweep(void)
{
	long n = 0;
	int sg, mode, hn, nf, pend, hk, ek, rep;
	for(sg = 0; sg < N_SIGN; sg++) for(mode = 0; mode < N_MODE; mode++) for(hn = 0; hn < N_NAN; hn++)
	for(nf = 0; nf < N_NF; nf++) for(pend = 0; pend < N_PENDING; pend++) for(hk = 0; hk < N_HKIND; hk++)
	for(ek = 0; ek < N_EPS; ek++) for(rep = 0; rep < N_REP; rep++) {
		const double dir = sg ? -1.0 : 1.0;
		old_consts B;
		double t = uni(-50.0, 50.0), left = logu(1e-3, 1e3), h, eps, thr;
		B.delta = logu(1e-9, 1e-2);
		B.h_min = logu(1e-12, 1e-6);
		B.delta_mode = mode ? DELTA_GLOBAL : DELTA_LOCAL;
		B.handle_nan = hn;
		B.final_time = t + dir * left;
		left = B.final_time - t;                       /* as the controller forms it */
		switch(hk) {
		case 0: h = left / uni(0.5, 4.0); break;                         /* ordinary: new_h against what is left */
		case 1: h = dir * B.h_min * uni(0.01, 0.99); break;              /* |h| < h_min */
		case 2: h = left * 1e-11 * (1.0 - 0x1p-40); break;               /* h/(final-t) below 1e-11 */
		case 3: h = left * 1e-11 * (1.0 + 0x1p-40); break;               /* ... above */
		case 4: h = nextafter(B.final_time, t) - t; break;               /* t+h an ulp or so short of final_time */
		case 5: h = left; break;                                         /* at it */
		case 6: h = nextafter(B.final_time, B.final_time + dir) - t; break;   /* past it */
		default:                                                         /* at it with |h| < h_min: accepted whatever */
			t = 0.0;                                                     /* the error norm, and with an infinite one */
			h = B.final_time = dir * B.h_min * uni(0.01, 0.99);          /* new_h = 0 = |final_time - (t+h)| */
			break;
		}
		/* the error norm that scales to delta */
		thr = B.delta_mode == DELTA_LOCAL ? B.delta / fabs(h / 3.0) : B.delta;
		switch(ek) {
		case 0: eps = 0.0; break;
		case 1: eps = 0x1p-1074; break;                                  /* subnormal */
		case 2: eps = nextafter(thr, 0.0); break;                        /* just below delta */
		case 3: eps = thr; break;
		case 4: eps = nextafter(thr, INFINITY); break;
		case 5: eps = thr * (1.0 + 0x1p-30); break;                      /* above */
		case 6: eps = 1e300; break;
		case 7: eps = INFINITY; break;
		case 8: eps = NAN; break;
		case 9: eps = thr * logu(1e-6, 1.0); break;                      /* accepted, any growth */
		case 10: eps = thr * logu(1.0, 1e6); break;                      /* rejected, any shrink */
		default: eps = thr * uni(0.2, 0.5); break;                       /* new_h about h: the NEXTFINISH edge */
		}
		one_case(&B, t, h, eps, nf, pend ? RKA_CMD_FINISHED : 0);
		n++;
	}
	return n;
}

/* ---- 3: chains ------------------------------------------------------------------------------ */

#define N_CHAIN 16

/* scripted error norm of attempt i, as a multiple of the accept threshold: accepts, a rejection, a
   NaN retreat (non-finite flag, handle_nan on), then the run-in */
static double script(int i, int * nf)
{
	*nf = i == 5;
	if(i < 3) return 0.5;
	if(i == 3) return 4.0;
	if(i == 4) return 0.9;
	if(i == 5) return 0.5;
	return i % 7 == 0 ? 1.5 : 0.05 + 0.1 * (i % 5);
}

static long chains(void)
{
	long total = 0;
	int ci;
	for(ci = 0; ci < N_CHAIN; ci++) {
		const double dir = ci & 1 ? -1.0 : 1.0;
		old_consts B;
		pft_stepctl_consts k;
		old_loop o;
		pft_step a = {0.0, 0.0, 0};
		double t, h;
		int i, done = 0;
		long steps = 0, attempted = 0;
		B.delta = logu(1e-8, 1e-3);
		B.h_min = 1e-10;
		B.delta_mode = ci & 2 ? DELTA_GLOBAL : DELTA_LOCAL;
		B.handle_nan = 1;
		t = uni(-5.0, 5.0);
		B.final_time = t + dir * uni(0.5, 3.0);
		h = (B.final_time - t) / uni(30.0, 60.0);
		k = consts_of(&B);
		memset(&o, 0, sizeof o);
		o.t = t; o.h = h; o.sys_t = NEVER; o.sys_h = NEVER;
		a.t = t; a.h = h;
		for(i = 0; i < 10000 && !done; i++) {
			int nf;
			const double mult = script(i, &nf);
			const double eps = mult * (B.delta_mode == DELTA_LOCAL ? B.delta / fabs(o.h / 3.0) : B.delta);
			pft_step s;
			double new_h;
			int cmd;
			old_body(&B, &o, eps, nf);
			cmd = pft_stepctl_judge(k, a, eps, nf, &new_h);
			s = pft_stepctl_advance(k, a, cmd, new_h);
			attempted++;
			if(((cmd & RKA_CMD_NAN) && (cmd & RKA_CMD_h_TOO_SMALL)) || o.ret) fail("chain: -4", &B, a.t, a.h, eps, nf, a.command);
			if(pft_stepctl_accepted(cmd)) {
				steps++;
				if(a.command & RKA_CMD_FINISHED) { a.t = s.t; done = 1; }
			}
			if(!done) a = s;
			if(done != o.ended || steps != o.steps || attempted != o.attempted || !same(a.t, o.t) ||
			   (!done && (!same(a.h, o.h) || a.command != o.command)))
				fail("chain step", &B, a.t, a.h, eps, nf, a.command);
			total++;
		}
		if(!done || !same(a.t, B.final_time) || steps < 10 || attempted < steps + 2 || !o.last_nan)
			fail("chain end", &B, a.t, a.h, 0.0, 0, a.command);
	}
	return total;
}

/* ---- 4: the stage scalars ------------------------------------------------------------------- */

#define N_SCALARS 4000

static long scalars(void)
{
	long n = 0;
	int i, st;
	for(i = 0; i < N_SCALARS; i++) {
		const double t = uni(-100.0, 100.0), h = (i & 1 ? -1.0 : 1.0) * logu(1e-12, 1e3);
		const double h2 = h/2.0, h3 = h/3.0, h6 = h/6.0, h8 = h/8.0;            /* :355 */
		const double ts[7] = {0, t, t+h3, t+h3, t+h2, t+h, t+h};
		const double coef[7] = {0, h3, h6, h8, h, h3, 0.0};
		const double cin[7] = {0, h, h/3.0, h/6.0, h/8.0, h, h};
		for(st = 1; st <= 6; st++) {
			const pft_stage_scalars s = pft_stepctl_stage(st, t, h);
			if(!same(s.ts, ts[st]) || !same(s.coef, coef[st]) || !same(s.cin, cin[st])) {
				printf("MISMATCH stage scalars: stage %d t %a h %a\n", st, t, h);
				exit(1);
			}
			n++;
		}
	}
	return n;
}

int main(void)
{
	const long a = sweep(), b = chains(), c = scalars();
	if(a != (long)N_SIGN * N_MODE * N_NAN * N_NF * N_PENDING * N_HKIND * N_EPS * N_REP || c != 6L * N_SCALARS) {
		printf("MISMATCH counts\n");
		return 1;
	}
	printf("%ld %ld %ld\n", a, b, c);
	return 0;
}
