/* pft_stepctl.h -- the Merson step controller (RK_MPI_SAsolver_hybrid2.c:355, 493-503, 578-611, 626-668,
   743-761), stated once for the host's loops, the device's gate and the CPU test:
   plain C that is also C++ and HIP, the reference's operations in its order; build without contraction.
   oracle/pft_oracle.c states the controller on its own and never includes this. */
#ifndef PFT_STEPCTL_H
#define PFT_STEPCTL_H

#include <math.h>
#include "../../include/RK_MPI_SAsolver.h"   /* RKA_CMD_* */

#if defined(__HIPCC__)
#define PFT_SC_HD __host__ __device__ __forceinline__
#else
#define PFT_SC_HD static inline
#endif

/* stage 1..5 of the step (t, h), or 6, the speculative stage 1 of the next step: its time, its combine's
   coefficient (stage 5: x(t+h)'s) and that of the combine that made its input (the previous stage's) */
typedef struct pft_stage_scalars { double ts, coef, cin; } pft_stage_scalars;

PFT_SC_HD pft_stage_scalars pft_stepctl_stage(int stage, double t, double h)
{
	const double h3 = h / 3.0;   /* h2, h3, h6, h8 of :355, each where used (the order keeps the gated kernels' code) */
	pft_stage_scalars s;
	switch(stage) {
	case 1:  s.ts = t;            s.coef = h3;      s.cin = h;       break;   /* :373-389 */
	case 2:  s.coef = h / 6.0;    s.ts = t + h3;    s.cin = h3;      break;   /* :392-409 */
	case 3:  s.coef = h / 8.0;    s.ts = t + h3;    s.cin = h / 6.0; break;   /* :412-429 */
	case 4:  s.ts = t + h / 2.0;  s.coef = h;       s.cin = h / 8.0; break;   /* :432-450 */
	case 5:  s.ts = t + h;        s.coef = h3;      s.cin = h;       break;   /* :453, 507-524, 657-668 */
	default: s.ts = t + h;        s.coef = 0.0;     s.cin = h;       break;   /* 6: nothing combined */
	}
	return s;
}

/* x^0.2 rounded to nearest from a candidate c within 1 ulp (ocml's pow): c is checked
   against the midpoints m to its neighbours in double-double arithmetic, x^0.2 > m <=> x > m^5 (1 - 25 e ln m)
   with 0.2 = 1/5 + e, e = 2^-54 / 5.  Outside a safe range c stays (the host's check of a gated step catches it). */
typedef struct pft_dd { double hi, lo; } pft_dd;
PFT_SC_HD pft_dd dd_norm(double a, double b)
{
	const double s = a + b;
	const pft_dd r = {s, b - (s - a)};
	return r;
}
PFT_SC_HD pft_dd dd_mul(pft_dd a, pft_dd b)
{
	const double p = a.hi * b.hi;
	double e = fma(a.hi, b.hi, -p);
	e += a.hi * b.lo + a.lo * b.hi;
	return dd_norm(p, e);
}
/* sign of x - m^(1/0.2) for the midpoint m = c + d (d = half the gap to a neighbour of c) */
PFT_SC_HD int pow02_side(double x, double c, double d, double k)
{
	const pft_dd m = {c, d};
	const pft_dd m2 = dd_mul(m, m), m4 = dd_mul(m2, m2), m5 = dd_mul(m4, m);
	const double corr = -(m5.hi * k) + m5.lo;   /* T = m5 (1 - k): m5.hi - m5.hi k + m5.lo */
	const double s = x - m5.hi;                 /* exact when x and m5.hi are close (Sterbenz) */
	const double r = s - corr;
	return r > 0.0 ? 1 : (r < 0.0 ? -1 : 0);
}
PFT_SC_HD double pow02_fix(double x, double c)
{
	if(!(x > 0x1p-900 && x < 0x1p900) || !(c > 0.0 && c < 0x1p200)) return c;
	const double k = 25.0 * (0x1p-54 / 5.0) * log(c);
	const double up = nextafter(c, INFINITY), dn = nextafter(c, 0.0);
	if(pow02_side(x, c, 0.5 * (up - c), k) > 0) return up;
	if(pow02_side(x, c, 0.5 * (dn - c), k) < 0) return dn;
	return c;
}
/* the controller's x^0.2, the one operation IEEE does not round: the C library's on the host, ocml's corrected */
PFT_SC_HD double pft_stepctl_pow02(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return pow02_fix(x, pow(x, 0.2));
#else
	return pow(x, 0.2);
#endif
}

/* a solve's constants (delta_local: delta_mode == DELTA_LOCAL) */
typedef struct pft_stepctl_consts { double final_time, delta, h_min; int delta_local, handle_nan; } pft_stepctl_consts;

/* an attempt: its t and h and the command pending on it (0 or RKA_CMD_FINISHED) */
typedef struct pft_step { double t, h; int command; } pft_step;

/* the attempt a judged by its error norm eps (nonfinite: its flag): its command with the judged bits, and *new_h */
PFT_SC_HD int pft_stepctl_judge(pft_stepctl_consts k, pft_step a, double eps, int nonfinite, double * new_h)
{
	const double h3 = a.h / 3.0;
	if(k.handle_nan && nonfinite) {                                          /* :493-503 */
		a.command |= RKA_CMD_NAN;
		if(a.h / (k.final_time - a.t) < 1e-11) a.command |= RKA_CMD_h_TOO_SMALL;
	}
	if(k.delta_local) eps *= fabs(h3);                                       /* :578 */
	*new_h = ((eps > 0.0) ? pft_stepctl_pow02((k.delta / eps)) * 0.8 : 2.0) * a.h;   /* :580 */
	if(eps < k.delta || fabs(a.h) < k.h_min) {                               /* :599-611 */
		a.command |= RKA_CMD_UPDATE;
		if(fabs(k.final_time - (a.t + a.h)) <= fabs(*new_h)) a.command |= RKA_CMD_NEXTFINISH;
	}
	return a.command;
}

/* x(t+h) becomes x; with NEXTFINISH besides, system->h keeps new_h, the step size to go on with */
PFT_SC_HD int pft_stepctl_accepted(int command) { return !(command & RKA_CMD_NAN) && (command & RKA_CMD_UPDATE); }

/* the attempt that follows a, judged as command and new_h (a gated launch's t and h, on the device) */
PFT_SC_HD pft_step pft_stepctl_advance(pft_stepctl_consts k, pft_step a, int command, double new_h)
{
	a.command = 0;
	if(command & RKA_CMD_NAN) { a.h /= 10; return a; }                       /* :626-646 */
	if(command & RKA_CMD_UPDATE) a.t += a.h;                                 /* :651-652 */
	if(command & RKA_CMD_NEXTFINISH) { a.h = k.final_time - a.t; a.command = RKA_CMD_FINISHED; }   /* :743-761 */
	else a.h = new_h;
	return a;
}

#endif
