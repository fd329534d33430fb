/* tests/native/cosh_check.c -- TEST INFRASTRUCTURE: libpft's restated cosh
   (porousfreezethaw_amd/csrc/pft_cosh.h, calc_mode 2's on the device) against (a) known answers of
   x86-64 glibc's cosh with the FMA build of exp, committed below as bit patterns, and (b) the
   running C library on n pseudo-random arguments.  Prints
       n  known answers pft_cosh misses  known answers the C library misses  mismatches of (b)
   Built and run by tests/test_cosh.py:
     gcc -O2 -std=c99 -ffp-contract=off -fno-fast-math cosh_check.c -lm && ./a.out n
   and once more with -fsanitize=address,undefined (also `make cosh-selftest`). */
#define _DEFAULT_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../porousfreezethaw_amd/csrc/pft_cosh.h"

/* { bits of x, bits of cosh(x) }.  The first five separate the FMA build of exp from the unfused
   one (whose last digit is the one in brackets); then signed zeros, infinities, a NaN, 2^-60 and
   2^-55, and both neighbours of every boundary of e_cosh.c: 0.5 ln2 (high word 0x3fd62e43), 22,
   log(DBL_MAX) (high word 0x40862e42), the overflow threshold 0x408633ce 8fb9f87d; exp's own
   switch at 512; a few plain values. */
static const uint64_t known[][2] = {
	{0x405f7e9f7465b97aULL, 0x4b3ae19dc3f67767ULL},   /* 0x1.f7e9f7465b97ap+6 -> 0x1.ae19dc3f67767p+180 (..68) */
	{0x406ddaf1f257c317ULL, 0x5567dae02521478fULL},   /* 0x1.ddaf1f257c317p+7 -> 0x1.7dae02521478fp+343 (..8e) */
	{0x405951ae94546680ULL, 0x490146eecca308abULL},   /* 0x1.951ae94546680p+6 -> 0x1.146eecca308abp+145 (..aa) */
	{0x4064426f892433efULL, 0x4e7c5f4a777104fdULL},   /* 0x1.4426f892433efp+7 -> 0x1.c5f4a777104fdp+232 (..fc) */
	{0x3ff743b55fd17d60ULL, 0x40020e4b015d3679ULL},   /* 0x1.743b55fd17d60p+0 -> 0x1.20e4b015d3679p+1 (..7a) */
	{0x0000000000000000ULL, 0x3ff0000000000000ULL},   /* 0x0.0p+0 -> 0x1.0000000000000p+0 */
	{0x8000000000000000ULL, 0x3ff0000000000000ULL},   /* -0x0.0p+0 -> 0x1.0000000000000p+0 */
	{0x7ff0000000000000ULL, 0x7ff0000000000000ULL},   /* inf -> inf */
	{0xfff0000000000000ULL, 0x7ff0000000000000ULL},   /* -inf -> inf */
	{0x7ff8000000000000ULL, 0x7ff8000000000000ULL},   /* nan -> nan */
	{0x3c30000000000000ULL, 0x3ff0000000000000ULL},   /* 0x1.0000000000000p-60 -> 0x1.0000000000000p+0 */
	{0xbc30000000000000ULL, 0x3ff0000000000000ULL},   /* -0x1.0000000000000p-60 -> 0x1.0000000000000p+0 */
	{0x3c80000000000000ULL, 0x3ff0000000000000ULL},   /* 0x1.0000000000000p-55 -> 0x1.0000000000000p+0 */
	{0x3c7fffffffffffffULL, 0x3ff0000000000000ULL},   /* 0x1.fffffffffffffp-56 -> 0x1.0000000000000p+0 */
	{0x3fd62e42ffffffffULL, 0x3ff0f876ccf6901dULL},   /* 0x1.62e42ffffffffp-2 -> 0x1.0f876ccf6901dp+0 */
	{0x3fd62e4300000000ULL, 0x3ff0f876ccf6901cULL},   /* 0x1.62e4300000000p-2 -> 0x1.0f876ccf6901cp+0 */
	{0x3fd62e4300000001ULL, 0x3ff0f876ccf6901dULL},   /* 0x1.62e4300000001p-2 -> 0x1.0f876ccf6901dp+0 */
	{0xbfd62e42ffffffffULL, 0x3ff0f876ccf6901dULL},   /* -0x1.62e42ffffffffp-2 -> 0x1.0f876ccf6901dp+0 */
	{0xbfd62e4300000000ULL, 0x3ff0f876ccf6901cULL},   /* -0x1.62e4300000000p-2 -> 0x1.0f876ccf6901cp+0 */
	{0xbfd62e4300000001ULL, 0x3ff0f876ccf6901dULL},   /* -0x1.62e4300000001p-2 -> 0x1.0f876ccf6901dp+0 */
	{0x4035ffffffffffffULL, 0x41dab5adb9c435e5ULL},   /* 0x1.5ffffffffffffp+4 -> 0x1.ab5adb9c435e5p+30 */
	{0x4036000000000000ULL, 0x41dab5adb9c43600ULL},   /* 0x1.6000000000000p+4 -> 0x1.ab5adb9c43600p+30 */
	{0x4036000000000001ULL, 0x41dab5adb9c4361aULL},   /* 0x1.6000000000001p+4 -> 0x1.ab5adb9c4361ap+30 */
	{0xc035ffffffffffffULL, 0x41dab5adb9c435e5ULL},   /* -0x1.5ffffffffffffp+4 -> 0x1.ab5adb9c435e5p+30 */
	{0xc036000000000000ULL, 0x41dab5adb9c43600ULL},   /* -0x1.6000000000000p+4 -> 0x1.ab5adb9c43600p+30 */
	{0xc036000000000001ULL, 0x41dab5adb9c4361aULL},   /* -0x1.6000000000001p+4 -> 0x1.ab5adb9c4361ap+30 */
	{0x40862e41ffffffffULL, 0x7fdffc045692fc9eULL},   /* 0x1.62e41ffffffffp+9 -> 0x1.ffc045692fc9ep+1022 */
	{0x40862e4200000000ULL, 0x7fdffc045693009eULL},   /* 0x1.62e4200000000p+9 -> 0x1.ffc045693009ep+1022 */
	{0x40862e4200000001ULL, 0x7fdffc045693049cULL},   /* 0x1.62e4200000001p+9 -> 0x1.ffc045693049cp+1022 */
	{0xc0862e41ffffffffULL, 0x7fdffc045692fc9eULL},   /* -0x1.62e41ffffffffp+9 -> 0x1.ffc045692fc9ep+1022 */
	{0xc0862e4200000000ULL, 0x7fdffc045693009eULL},   /* -0x1.62e4200000000p+9 -> 0x1.ffc045693009ep+1022 */
	{0xc0862e4200000001ULL, 0x7fdffc045693049cULL},   /* -0x1.62e4200000001p+9 -> 0x1.ffc045693049cp+1022 */
	{0x408633ce8fb9f87cULL, 0x7feffffffffff93bULL},   /* 0x1.633ce8fb9f87cp+9 -> 0x1.ffffffffff93bp+1023 */
	{0x408633ce8fb9f87dULL, 0x7feffffffffffd3bULL},   /* 0x1.633ce8fb9f87dp+9 -> 0x1.ffffffffffd3bp+1023 */
	{0x408633ce8fb9f87eULL, 0x7ff0000000000000ULL},   /* 0x1.633ce8fb9f87ep+9 -> inf */
	{0xc08633ce8fb9f87cULL, 0x7feffffffffff93bULL},   /* -0x1.633ce8fb9f87cp+9 -> 0x1.ffffffffff93bp+1023 */
	{0xc08633ce8fb9f87dULL, 0x7feffffffffffd3bULL},   /* -0x1.633ce8fb9f87dp+9 -> 0x1.ffffffffffd3bp+1023 */
	{0xc08633ce8fb9f87eULL, 0x7ff0000000000000ULL},   /* -0x1.633ce8fb9f87ep+9 -> inf */
	{0x3fd62e42fefa39efULL, 0x3ff0f876ccdf6cd9ULL},   /* 0x1.62e42fefa39efp-2 -> 0x1.0f876ccdf6cd9p+0 */
	{0x4086280000000000ULL, 0x7fcd422d2be5dc9bULL},   /* 0x1.6280000000000p+9 -> 0x1.d422d2be5dc9bp+1021 */
	{0x4086300000000000ULL, 0x7fe3e21a464507faULL},   /* 0x1.6300000000000p+9 -> 0x1.3e21a464507fap+1023 */
	{0xc086333333333333ULL, 0x7feda98a7371610aULL},   /* -0x1.6333333333333p+9 -> 0x1.da98a7371610ap+1023 */
	{0x3ff0000000000000ULL, 0x3ff8b07551d9f550ULL},   /* 0x1.0000000000000p+0 -> 0x1.8b07551d9f550p+0 */
	{0xbff0000000000000ULL, 0x3ff8b07551d9f550ULL},   /* -0x1.0000000000000p+0 -> 0x1.8b07551d9f550p+0 */
	{0x4080000000000000ULL, 0x6e09476504ba852eULL},   /* 0x1.0000000000000p+9 -> 0x1.9476504ba852ep+737 */
	{0x407fffffffe5280dULL, 0x6e094764da5151e1ULL},   /* 0x1.fffffffe5280dp+8 -> 0x1.94764da5151e1p+737 */
	{0x4090000000000000ULL, 0x7ff0000000000000ULL},   /* 0x1.0000000000000p+10 -> inf */
	{0xc044000000000000ULL, 0x437a220d397972ebULL},   /* -0x1.4000000000000p+5 -> 0x1.a220d397972ebp+56 */
	{0x4044000000000000ULL, 0x437a220d397972ebULL},   /* 0x1.4000000000000p+5 -> 0x1.a220d397972ebp+56 */
};

/* equal bit for bit, any NaN equal to any NaN */
static int same(double a, double b)
{
	if(a != a || b != b) return a != a && b != b;
	return memcmp(&a, &b, 8) == 0;
}

static uint64_t splitmix64(uint64_t i)
{
	uint64_t b = i + 0x9E3779B97F4A7C15ULL;
	b = (b ^ (b >> 30)) * 0xBF58476D1CE4E5B9ULL;
	b = (b ^ (b >> 27)) * 0x94D049BB133111EBULL;
	return b ^ (b >> 31);
}

int main(int argc, char ** argv)
{
	const long n = argc > 1 ? atol(argv[1]) : 1000000;
	const int nknown = (int)(sizeof(known) / sizeof(known[0]));
	long bad = 0, bad_known = 0, bad_known_libm = 0, i;
	for(i = 0; i < nknown; i++) {
		const double x = pft_from_bits(known[i][0]), y = pft_from_bits(known[i][1]);
		if(!same(pft_cosh(x), y)) {
			bad_known++;
			fprintf(stderr, "pft_cosh(%a) = %a, expected %a\n", x, pft_cosh(x), y);
		}
		if(!same(cosh(x), y)) bad_known_libm++;
	}
	srand48(20261020);
	for(i = 0; i < n; i++) {
		double x;
		switch(i % 8) {
			case 0: x = (drand48() * 2 - 1) * 25; break;
			case 1: x = (drand48() * 2 - 1) * 2; break;
			case 2: x = drand48() * 0.7; break;                           /* the 0.5 ln2 switch */
			case 3: x = drand48() * 720; break;                           /* every range, overflow */
			case 4: x = -drand48() * 300; break;
			case 5: x = (drand48() * 2 - 1) * ldexp(1.0, -(int)(drand48() * 70)); break;
			case 6: x = 709.7 + drand48() * 0.9; break;                   /* log(DBL_MAX) .. overflow */
			default: x = pft_from_bits(splitmix64((uint64_t)i)); break;   /* any bit pattern */
		}
		if(!same(pft_cosh(x), cosh(x))) {
			if(bad++ < 10) fprintf(stderr, "pft_cosh(%a) = %a, cosh %a\n", x, pft_cosh(x), cosh(x));
		}
	}
	printf("%ld %ld %ld %ld\n", n, bad_known, bad_known_libm, bad);
	return 0;
}
