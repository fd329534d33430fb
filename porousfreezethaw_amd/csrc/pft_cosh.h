/*
 * pft_cosh.h -- cosh() exactly as the host's C library computes it, for calc_mode 2's
 * dp/du = -gamma/2 / cosh^2(gamma (u - u*)) (equation.c:835-874).  Compiled both as C (gcc, the CPU
 * check tests/test_cosh.py and the host twin pft_cosh_host) and as HIP device code
 * (pft_kernels.hip); always without contraction (-ffp-contract=off): every fused operation below
 * is written out as __builtin_fma (v_fma_f64 on the device, a correctly rounded fma on the host).
 *
 * "The C library's cosh" is that of x86-64 glibc 2.28 and later on a processor with FMA, which is
 * what produced the golden vectors: fdlibm's e_cosh.c on top of fdlibm's expm1 (pft_tanh.h) below
 * 0.5 ln2 and of the table-driven exp above it, and glibc's multiarch exp resolves to the build
 * compiled with contraction.  exp is restated from the published algorithm (exp.c of Arm's
 * optimized routines, N = 128, the order-5 polynomial):
 *     kd = round(x 128/ln2) by adding 0x1.8p52, k = its integer
 *     r  = x - kd ln2/128 in hi/lo parts,   |r| <= ln2/256
 *     2^(k/128) = scale (1 + tail), both from the table entry k % 128 (scale's exponent by
 *                 adding k's upper bits to the entry's second word)
 *     exp(x) = scale + scale (tail + r + r^2 (C2 + r C3) + r^4 (C4 + r C5))
 * with the fused operations exactly where that build has them; a restatement without them
 * differs from the C library in 7 671 of 11 475 081 results.  The table is regenerated from
 * first principles by scripts/gen_exp_table.py (2^(k/128) at 200 bits), not taken from a binary.
 * The CPU test compares pft_cosh with the C library on 10^7 arguments: equal bit for bit.
 * Attribution: e_cosh.c and expm1 are fdlibm's (Sun Microsystems, 1993); the exp algorithm and
 * its constants are Arm's optimized routines' (Arm Ltd., 2018, MIT licence); both as carried in
 * the GNU C Library.  None of the reference project's code is involved.
 */
#ifndef PFT_COSH_H
#define PFT_COSH_H

#include "pft_tanh.h"

/* entry k: { bits of tail, bits of scale - (k << 45) }, 2^(k/128) = scale (1 + tail) */
typedef struct {
	uint64_t tail, sbits;
} pft_exp_entry;

#define PFT_EXP_TAB_INIT \
	{0x0000000000000000ULL, 0x3ff0000000000000ULL}, {0x3c9b3b4f1a88bf6eULL, 0x3feff63da9fb3335ULL}, \
	{0xbc7160139cd8dc5dULL, 0x3fefec9a3e778061ULL}, {0xbc905e7a108766d1ULL, 0x3fefe315e86e7f85ULL}, \
	{0x3c8cd2523567f613ULL, 0x3fefd9b0d3158574ULL}, {0xbc8bce8023f98efaULL, 0x3fefd06b29ddf6deULL}, \
	{0x3c60f74e61e6c861ULL, 0x3fefc74518759bc8ULL}, {0x3c90a3e45b33d399ULL, 0x3fefbe3ecac6f383ULL}, \
	{0x3c979aa65d837b6dULL, 0x3fefb5586cf9890fULL}, {0x3c8eb51a92fdeffcULL, 0x3fefac922b7247f7ULL}, \
	{0x3c3ebe3d702f9cd1ULL, 0x3fefa3ec32d3d1a2ULL}, {0xbc6a033489906e0bULL, 0x3fef9b66affed31bULL}, \
	{0xbc9556522a2fbd0eULL, 0x3fef9301d0125b51ULL}, {0xbc5080ef8c4eea55ULL, 0x3fef8abdc06c31ccULL}, \
	{0xbc91c923b9d5f416ULL, 0x3fef829aaea92de0ULL}, {0x3c80d3e3e95c55afULL, 0x3fef7a98c8a58e51ULL}, \
	{0xbc801b15eaa59348ULL, 0x3fef72b83c7d517bULL}, {0xbc8f1ff055de323dULL, 0x3fef6af9388c8deaULL}, \
	{0x3c8b898c3f1353bfULL, 0x3fef635beb6fcb75ULL}, {0xbc96d99c7611eb26ULL, 0x3fef5be084045cd4ULL}, \
	{0x3c9aecf73e3a2f60ULL, 0x3fef54873168b9aaULL}, {0xbc8fe782cb86389dULL, 0x3fef4d5022fcd91dULL}, \
	{0x3c8a6f4144a6c38dULL, 0x3fef463b88628cd6ULL}, {0x3c807a05b0e4047dULL, 0x3fef3f49917ddc96ULL}, \
	{0x3c968efde3a8a894ULL, 0x3fef387a6e756238ULL}, {0x3c875e18f274487dULL, 0x3fef31ce4fb2a63fULL}, \
	{0x3c80472b981fe7f2ULL, 0x3fef2b4565e27cddULL}, {0xbc96b87b3f71085eULL, 0x3fef24dfe1f56381ULL}, \
	{0x3c82f7e16d09ab31ULL, 0x3fef1e9df51fdee1ULL}, {0xbc3d219b1a6fbffaULL, 0x3fef187fd0dad990ULL}, \
	{0x3c8b3782720c0ab4ULL, 0x3fef1285a6e4030bULL}, {0x3c6e149289cecb8fULL, 0x3fef0cafa93e2f56ULL}, \
	{0x3c834d754db0abb6ULL, 0x3fef06fe0a31b715ULL}, {0x3c864201e2ac744cULL, 0x3fef0170fc4cd831ULL}, \
	{0x3c8fdd395dd3f84aULL, 0x3feefc08b26416ffULL}, {0xbc86a3803b8e5b04ULL, 0x3feef6c55f929ff1ULL}, \
	{0xbc924aedcc4b5068ULL, 0x3feef1a7373aa9cbULL}, {0xbc9907f81b512d8eULL, 0x3feeecae6d05d866ULL}, \
	{0xbc71d1e83e9436d2ULL, 0x3feee7db34e59ff7ULL}, {0xbc991919b3ce1b15ULL, 0x3feee32dc313a8e5ULL}, \
	{0x3c859f48a72a4c6dULL, 0x3feedea64c123422ULL}, {0xbc9312607a28698aULL, 0x3feeda4504ac801cULL}, \
	{0xbc58a78f4817895bULL, 0x3feed60a21f72e2aULL}, {0xbc7c2c9b67499a1bULL, 0x3feed1f5d950a897ULL}, \
	{0x3c4363ed60c2ac11ULL, 0x3feece086061892dULL}, {0x3c9666093b0664efULL, 0x3feeca41ed1d0057ULL}, \
	{0x3c6ecce1daa10379ULL, 0x3feec6a2b5c13cd0ULL}, {0x3c93ff8e3f0f1230ULL, 0x3feec32af0d7d3deULL}, \
	{0x3c7690cebb7aafb0ULL, 0x3feebfdad5362a27ULL}, {0x3c931dbdeb54e077ULL, 0x3feebcb299fddd0dULL}, \
	{0xbc8f94340071a38eULL, 0x3feeb9b2769d2ca7ULL}, {0xbc87deccdc93a349ULL, 0x3feeb6daa2cf6642ULL}, \
	{0xbc78dec6bd0f385fULL, 0x3feeb42b569d4f82ULL}, {0xbc861246ec7b5cf6ULL, 0x3feeb1a4ca5d920fULL}, \
	{0x3c93350518fdd78eULL, 0x3feeaf4736b527daULL}, {0x3c7b98b72f8a9b05ULL, 0x3feead12d497c7fdULL}, \
	{0x3c9063e1e21c5409ULL, 0x3feeab07dd485429ULL}, {0x3c34c7855019c6eaULL, 0x3feea9268a5946b7ULL}, \
	{0x3c9432e62b64c035ULL, 0x3feea76f15ad2148ULL}, {0xbc8ce44a6199769fULL, 0x3feea5e1b976dc09ULL}, \
	{0xbc8c33c53bef4da8ULL, 0x3feea47eb03a5585ULL}, {0xbc845378892be9aeULL, 0x3feea34634ccc320ULL}, \
	{0xbc93cedd78565858ULL, 0x3feea23882552225ULL}, {0x3c5710aa807e1964ULL, 0x3feea155d44ca973ULL}, \
	{0xbc93b3efbf5e2228ULL, 0x3feea09e667f3bcdULL}, {0xbc6a12ad8734b982ULL, 0x3feea012750bdabfULL}, \
	{0xbc6367efb86da9eeULL, 0x3fee9fb23c651a2fULL}, {0xbc80dc3d54e08851ULL, 0x3fee9f7df9519484ULL}, \
	{0xbc781f647e5a3ecfULL, 0x3fee9f75e8ec5f74ULL}, {0xbc86ee4ac08b7db0ULL, 0x3fee9f9a48a58174ULL}, \
	{0xbc8619321e55e68aULL, 0x3fee9feb564267c9ULL}, {0x3c909ccb5e09d4d3ULL, 0x3feea0694fde5d3fULL}, \
	{0xbc7b32dcb94da51dULL, 0x3feea11473eb0187ULL}, {0x3c94ecfd5467c06bULL, 0x3feea1ed0130c132ULL}, \
	{0x3c65ebe1abd66c55ULL, 0x3feea2f336cf4e62ULL}, {0xbc88a1c52fb3cf42ULL, 0x3feea427543e1a12ULL}, \
	{0xbc9369b6f13b3734ULL, 0x3feea589994cce13ULL}, {0xbc805e843a19ff1eULL, 0x3feea71a4623c7adULL}, \
	{0xbc94d450d872576eULL, 0x3feea8d99b4492edULL}, {0x3c90ad675b0e8a00ULL, 0x3feeaac7d98a6699ULL}, \
	{0x3c8db72fc1f0eab4ULL, 0x3feeace5422aa0dbULL}, {0xbc65b6609cc5e7ffULL, 0x3feeaf3216b5448cULL}, \
	{0x3c7bf68359f35f44ULL, 0x3feeb1ae99157736ULL}, {0xbc93091fa71e3d83ULL, 0x3feeb45b0b91ffc6ULL}, \
	{0xbc5da9b88b6c1e29ULL, 0x3feeb737b0cdc5e5ULL}, {0xbc6c23f97c90b959ULL, 0x3feeba44cbc8520fULL}, \
	{0xbc92434322f4f9aaULL, 0x3feebd829fde4e50ULL}, {0xbc85ca6cd7668e4bULL, 0x3feec0f170ca07baULL}, \
	{0x3c71affc2b91ce27ULL, 0x3feec49182a3f090ULL}, {0x3c6dd235e10a73bbULL, 0x3feec86319e32323ULL}, \
	{0xbc87c50422622263ULL, 0x3feecc667b5de565ULL}, {0x3c8b1c86e3e231d5ULL, 0x3feed09bec4a2d33ULL}, \
	{0xbc91bbd1d3bcbb15ULL, 0x3feed503b23e255dULL}, {0x3c90cc319cee31d2ULL, 0x3feed99e1330b358ULL}, \
	{0x3c8469846e735ab3ULL, 0x3feede6b5579fdbfULL}, {0xbc82dfcd978e9db4ULL, 0x3feee36bbfd3f37aULL}, \
	{0x3c8c1a7792cb3387ULL, 0x3feee89f995ad3adULL}, {0xbc907b8f4ad1d9faULL, 0x3feeee07298db666ULL}, \
	{0xbc55c3d956dcaebaULL, 0x3feef3a2b84f15fbULL}, {0xbc90a40e3da6f640ULL, 0x3feef9728de5593aULL}, \
	{0xbc68d6f438ad9334ULL, 0x3feeff76f2fb5e47ULL}, {0xbc91eee26b588a35ULL, 0x3fef05b030a1064aULL}, \
	{0x3c74ffd70a5fddcdULL, 0x3fef0c1e904bc1d2ULL}, {0xbc91bdfbfa9298acULL, 0x3fef12c25bd71e09ULL}, \
	{0x3c736eae30af0cb3ULL, 0x3fef199bdd85529cULL}, {0x3c8ee3325c9ffd94ULL, 0x3fef20ab5fffd07aULL}, \
	{0x3c84e08fd10959acULL, 0x3fef27f12e57d14bULL}, {0x3c63cdaf384e1a67ULL, 0x3fef2f6d9406e7b5ULL}, \
	{0x3c676b2c6c921968ULL, 0x3fef3720dcef9069ULL}, {0xbc808a1883ccb5d2ULL, 0x3fef3f0b555dc3faULL}, \
	{0xbc8fad5d3ffffa6fULL, 0x3fef472d4a07897cULL}, {0xbc900dae3875a949ULL, 0x3fef4f87080d89f2ULL}, \
	{0x3c74a385a63d07a7ULL, 0x3fef5818dcfba487ULL}, {0xbc82919e2040220fULL, 0x3fef60e316c98398ULL}, \
	{0x3c8e5a50d5c192acULL, 0x3fef69e603db3285ULL}, {0x3c843a59ac016b4bULL, 0x3fef7321f301b460ULL}, \
	{0xbc82d52107b43e1fULL, 0x3fef7c97337b9b5fULL}, {0xbc892ab93b470dc9ULL, 0x3fef864614f5a129ULL}, \
	{0x3c74b604603a88d3ULL, 0x3fef902ee78b3ff6ULL}, {0x3c83c5ec519d7271ULL, 0x3fef9a51fbc74c83ULL}, \
	{0xbc8ff7128fd391f0ULL, 0x3fefa4afa2a490daULL}, {0xbc8dae98e223747dULL, 0x3fefaf482d8e67f1ULL}, \
	{0x3c8ec3bc41aa2008ULL, 0x3fefba1bee615a27ULL}, {0x3c842b94c3a9eb32ULL, 0x3fefc52b376bba97ULL}, \
	{0x3c8a64a931d185eeULL, 0x3fefd0765b6e4540ULL}, {0xbc8e37bae43be3edULL, 0x3fefdbfdad9cbe14ULL}, \
	{0x3c77893b4d91cd9dULL, 0x3fefe7c1819e90d8ULL}, {0x3c5305c14160cc89ULL, 0x3feff3c22b8f71f1ULL}

/* 2 KiB; 16-byte entries, so that the device fetches both words with one global_load_dwordx4 */
#if defined(__HIPCC__)
static __device__ const pft_exp_entry pft_exp_tab_dev[128] __attribute__((aligned(16))) = {PFT_EXP_TAB_INIT};
#endif
static const pft_exp_entry pft_exp_tab[128] __attribute__((aligned(16))) = {PFT_EXP_TAB_INIT};

static inline PFT_HD double pft_from_bits(uint64_t u)
{
	double x;
	memcpy(&x, &u, 8);
	return x;
}

/* exp(x) for the arguments cosh hands it, 0.5 ln2 < x < 710.5, without a branch.  From 512 on the
 * scale's exponent may exceed the format's, so it is built 2^1009 too small and the result
 * multiplied by 2^1009 (the algorithm's special case for k > 0; below 512 the multiplier is 1.0,
 * which is exact).  The special case's other half (k < 0, results near or below the subnormals),
 * the shortcut 1 + x for |x| < 2^-54 and the checks for overflow, infinities and NaNs are not
 * here: no argument of cosh's reaches them.  For any other x the result is unspecified but the
 * table index stays within 0 .. 127. */
static inline PFT_HD double pft_exp_pos(double x)
{
	const double InvLn2N = 0x1.71547652b82fep0 * 128, Shift = 0x1.8p52;
	const double NegLn2hiN = -0x1.62e42fefa0000p-8, NegLn2loN = -0x1.cf79abc9e3b3ap-47;
	const double C2 = 0x1.ffffffffffdbdp-2, C3 = 0x1.555555555543cp-3, C4 = 0x1.55555cf172b91p-5,
	             C5 = 0x1.1111167a4d017p-7;
	double kd = InvLn2N * x + Shift;             /* not fused (fusing it changes nothing) */
	uint64_t ki;
	memcpy(&ki, &kd, 8);
	kd -= Shift;
	const double r = __builtin_fma(kd, NegLn2loN, __builtin_fma(kd, NegLn2hiN, x));
#if defined(__HIP_DEVICE_COMPILE__)
	const pft_exp_entry e = pft_exp_tab_dev[ki & 127u];
#else
	const pft_exp_entry e = pft_exp_tab[ki & 127u];
#endif
	const int big = x >= 512.0;
	const double scale = pft_from_bits(e.sbits + (ki << 45) - (big ? (uint64_t)1009 << 52 : 0));
	const double r2 = r * r;
	const double tmp = __builtin_fma(r2 * r2, __builtin_fma(r, C5, C4),
	                                 __builtin_fma(r2, __builtin_fma(r, C3, C2), pft_from_bits(e.tail) + r));
	return (big ? 0x1p1009 : 1.0) * __builtin_fma(scale, tmp, scale);
}

/* cosh(x), fdlibm e_cosh.c (glibc sysdeps/ieee754/dbl-64/e_cosh.c) */
static inline PFT_HD double pft_cosh(double x)
{
	const double one = 1.0, half = 0.5, huge = 1.0e300;
	const uint32_t ix = pft_hi32(x) & 0x7fffffffu, lx = pft_lo32(x);
	const double ax = pft_with_hi32(x, ix);      /* |x| */
	double t, w;
	if(ix < 0x3fd62e43u) {                       /* |x| < 0.5 ln2: 1 + expm1(|x|)^2 / (2 exp(|x|)) */
		t = pft_expm1(ax);
		w = one + t;
		if(ix < 0x3c800000u) return w;           /* |x| < 2^-55: 1 */
		return one + (t * t) / (w + w);
	}
	if(ix >= 0x7ff00000u) return x * x;          /* inf, NaN */
	if(ix > 0x408633ceu || (ix == 0x408633ceu && lx > 0x8fb9f87du)) return huge * huge;   /* overflow */
	/* one exp for the three ranges: of |x| / 2 from log(DBL_MAX) to the overflow threshold */
	const int top = ix >= 0x40862e42u;
	t = pft_exp_pos(top ? half * ax : ax);
	if(ix < 0x40360000u) return half * t + half / t;   /* |x| < 22: (exp(|x|) + 1 / exp(|x|)) / 2 */
	if(!top) return half * t;                    /* |x| < log(DBL_MAX) */
	w = half * t;
	return w * t;
}

#endif
