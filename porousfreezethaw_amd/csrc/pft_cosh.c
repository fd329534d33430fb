/* pft_cosh.c -- the host twin of the device's cosh: pft_cosh.h compiled by gcc without contraction,
   for the tests that compare the device function with it and with the C library */
#include "../../include/pft_hip.h"
#include "pft_cosh.h"

int pft_cosh_host(const double * x, double * y, unsigned long long n)
{
	unsigned long long i;
	if(n && (!x || !y)) return -2;
	for(i = 0; i < n; i++) y[i] = pft_cosh(x[i]);
	return 0;
}
