/*
 * pft_region_selftest.c -- a stand-alone host program over the region code of pft_io.c for a run
 * under the host sanitizers (make -C porousfreezethaw_amd region-selftest: -fsanitize=address,undefined;
 * no GPU, no Python):
 *   - pft_region_local, exhaustively: every total_n3 <= 9 cut into 1-4 slabs (the driver's
 *     decomposition, a slab of one plane or of none included) and every valid k triple, against a
 *     brute-force list of the selected planes each slab owns; the shares are disjoint, ordered and
 *     sum to count[2];
 *   - pft_region_check on the triples just outside the rules;
 *   - pft_region_image_host on a few shapes and regions against a plain triple loop over a padded
 *     array whose ghost cells hold other values, on every slab of 1-3;
 *   - a region dataset written slab by slab (create_region, region_ranges, write_image -- a slab
 *     with no share writes nothing) and read back with read_image against the single slab's image.
 * Exit status 0 when every case holds, 1 otherwise.
 */
#define _XOPEN_SOURCE 700
#include "../../include/pft_io.h"
#include "../../include/pft_comm.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

/* pft_snapshot_write's communicator (pft_comm.hip, not linked here): one rank */
pft_comm * pft_comm_current(void) { return NULL; }
int pft_comm_allreduce_max_i64(pft_comm * c, long long * v) { (void)c; (void)v; return 0; }

static long failures, cases;
#define CHECK(cond, what) do { cases++; if(!(cond)) { if(failures < 20) printf("FAIL %s (line %d)\n", what, __LINE__); failures++; } } while(0)

/* the driver's decomposition (intertrack.c:1780-1787), restated: the test's own copy */
static void slab_of(pft_grid * g, int n1, int n2, int total, int nprocs, int rank)
{
	int n = total / nprocs, f = rank * n;
	if(rank < total % nprocs) { n++; f += rank; } else f += total % nprocs;
	memset(g, 0, sizeof *g);
	g->n1 = n1; g->n2 = n2; g->n3 = n; g->total_n3 = total; g->first_row = f; g->rank = rank; g->nprocs = nprocs;
	g->L1 = 0.03; g->L2 = 0.05; g->L3 = 0.07;
}

static void local_exhaustive(void)
{
	int total, np, rank, start, count, stride;
	for(total = 1; total <= 9; total++)
		for(np = 1; np <= 4; np++)
			for(start = 0; start < total; start++)
				for(stride = 1; stride <= total + 1; stride++)
					for(count = 1; start + (count - 1) * stride < total; count++) {
						int sum = 0, next = 0;
						for(rank = 0; rank < np; rank++) {
							pft_grid g;
							pft_region r = {{0, 0, start}, {1, 1, count}, {1, 1, stride}};
							int kfirst = -7, kcount = -7, klocal = -7, m, bf = -1, bc = 0, bl = 0;
							slab_of(&g, 3, 2, total, np, rank);
							for(m = 0; m < count; m++) {
								const int k = start + m * stride;
								if(k >= g.first_row && k < g.first_row + g.n3) {
									if(!bc) { bf = m; bl = k - g.first_row; }
									bc++;
								}
							}
							CHECK(pft_region_local(&g, &r, &kfirst, &kcount, &klocal) == 0, "region_local rc");
							CHECK(kcount == bc, "kcount");
							if(bc) {
								CHECK(kfirst == bf && klocal == bl, "kfirst / klocal");
								CHECK(klocal >= 0 && klocal + (long)(kcount - 1) * stride < g.n3, "share inside the slab");
							}
							CHECK(kfirst == next, "shares ordered and contiguous");
							next = kfirst + kcount;
							sum += kcount;
							CHECK(pft_region_image_bytes(&g, &r) == 24u * (size_t)kcount, "image bytes");
						}
						CHECK(sum == count, "shares sum to the count");
					}
}

static void check_rules(void)
{
	pft_grid g;
	pft_region ok = {{1, 0, 2}, {3, 5, 2}, {2, 1, 3}};   /* i 1,3,5; j 0..4; k 2,5 */
	int a;
	slab_of(&g, 7, 5, 7, 1, 0);
	CHECK(pft_region_check(&g, &ok) == 0, "a valid region");
	for(a = 0; a < 3; a++) {
		pft_region r = ok;
		r.stride[a] = 0; CHECK(pft_region_check(&g, &r) == -2, "stride 0");
		r = ok; r.stride[a] = -1; CHECK(pft_region_check(&g, &r) == -2, "negative stride");
		r = ok; r.count[a] = 0; CHECK(pft_region_check(&g, &r) == -2, "count 0");
		r = ok; r.start[a] = -1; CHECK(pft_region_check(&g, &r) == -2, "negative start");
		r = ok; r.count[a] += 1;
		CHECK(pft_region_check(&g, &r) == -2, "one past the last cell");
		r = ok; r.start[a] = a == 0 ? 7 : a == 1 ? 5 : 7; r.count[a] = 1;
		CHECK(pft_region_check(&g, &r) == -2, "start past the grid");
		r = ok; r.start[a] = (a == 0 ? 7 : a == 1 ? 5 : 7) - 1; r.count[a] = 1; r.stride[a] = 1000;
		CHECK(pft_region_check(&g, &r) == 0, "the last cell alone, any stride");
	}
	CHECK(pft_region_check(NULL, &ok) == -2 && pft_region_check(&g, NULL) == -2, "NULL");
}

/* a padded slab array of the global function v(q, kglobal, j, i); ghost cells hold -1 - that */
static double value(int q, long k, long j, long i) { return (double)(((q * 1000 + k) * 1000 + j) * 1000 + i) + 0.25; }

static double * fill(const pft_grid * g)
{
	const long N1 = g->n1 + 4, N2 = g->n2 + 4, N3 = g->n3 + 4;
	double * x = (double *)malloc(sizeof(double) * 3 * (size_t)(N1 * N2 * N3));
	long q, k, j, i;
	if(!x) return NULL;
	for(q = 0; q < 3; q++) for(k = 0; k < N3; k++) for(j = 0; j < N2; j++) for(i = 0; i < N1; i++) {
		const int inside = k >= 2 && k < N3 - 2 && j >= 2 && j < N2 - 2 && i >= 2 && i < N1 - 2;
		const double v = value((int)q, g->first_row + k - 2, j - 2, i - 2);
		x[((q * N3 + k) * N2 + j) * N1 + i] = inside ? v : -1.0 - v;
	}
	return x;
}

static uint64_t be(double d) { uint64_t u; memcpy(&u, &d, 8); return __builtin_bswap64(u); }

static void images(const char * dir)
{
	static const int shapes[3][3] = {{7, 5, 7}, {8, 6, 5}, {33, 31, 9}};
	int sh, rg, np, rank;
	double param[PFT_PARAM_COUNT];
	pft_snapshot_info info;
	memset(&info, 0, sizeof info);
	for(rg = 0; rg < PFT_PARAM_COUNT; rg++) param[rg] = 1.0 + rg;
	pft_snapshot_title(info.title, sizeof info.title, "region selftest", 3.5);
	for(sh = 0; sh < 3; sh++) {
		const int n1 = shapes[sh][0], n2 = shapes[sh][1], n3 = shapes[sh][2];
		const pft_region regs[] = {
			{{0, 0, 0}, {n1, n2, n3}, {1, 1, 1}},                                       /* everything */
			{{n1 / 2, 0, 0}, {1, n2, n3}, {1, 1, 1}},                                   /* a y-z section */
			{{0, n2 / 2, 0}, {n1, 1, n3}, {1, 1, 1}},                                   /* an x-z section */
			{{1, 1, 1}, {(n1 - 1 + 1) / 2, (n2 - 1 + 2) / 3, (n3 - 1 + 1) / 2}, {2, 3, 2}},   /* strided */
			{{n1 - 2, n2 - 2, n3 - 2}, {2, 2, 2}, {1, 1, 1}},                           /* ends on the last cell */
			{{n1 - 1, n2 - 1, n3 - 1}, {1, 1, 1}, {5, 7, 9}},                           /* one cell */
			{{0, 0, 0}, {(n1 + 2) / 3, 1, (n3 + 4) / 5}, {3, n2, 5}},
		};
		for(rg = 0; rg < (int)(sizeof regs / sizeof regs[0]); rg++) {
			const pft_region * r = &regs[rg];
			const size_t words = (size_t)r->count[0] * r->count[1] * r->count[2];
			uint64_t * whole = (uint64_t *)malloc(24 * words), * back = (uint64_t *)malloc(24 * words);
			char path[300];
			pft_grid one;
			long q, k, j, i;
			size_t w = 0;
			slab_of(&one, n1, n2, n3, 1, 0);
			CHECK(pft_region_check(&one, r) == 0, "the test's region is valid");
			/* the plain triple loop */
			for(q = 0; q < 3; q++) for(k = 0; k < r->count[2]; k++) for(j = 0; j < r->count[1]; j++)
				for(i = 0; i < r->count[0]; i++)
					whole[w++] = be(value((int)q, r->start[2] + k * r->stride[2], r->start[1] + j * r->stride[1],
					                      r->start[0] + i * r->stride[0]));
			for(np = 1; np <= 3; np++) {
				snprintf(path, sizeof path, "%s/r_%d_%d_%d.ncd", dir, sh, rg, np);
				CHECK(pft_snapshot_create_region(path, &one, r, param, &info, np == 2 ? 2 : 0) == 0, "create_region");
				for(rank = np - 1; rank >= 0; rank--) {
					pft_grid g;
					pft_snapshot_ranges ranges;
					int kfirst, kcount, klocal;
					double * x;
					uint64_t * img;
					size_t mine, per = (size_t)r->count[0] * r->count[1];
					slab_of(&g, n1, n2, n3, np, rank);
					x = fill(&g);
					CHECK(pft_region_local(&g, r, &kfirst, &kcount, &klocal) == 0, "region_local");
					mine = per * (size_t)kcount;
					CHECK(pft_region_image_bytes(&g, r) == 24 * mine, "image bytes");
					img = (uint64_t *)malloc(24 * mine + 8);
					CHECK(x && img, "malloc");
					if(x && img) {
						img[3 * mine] = 0x5a5a5a5a5a5a5a5aULL;                 /* a guard word behind the image */
						CHECK(pft_region_image_host(&g, r, x, img) == 0, "image_host");
						CHECK(img[3 * mine] == 0x5a5a5a5a5a5a5a5aULL, "nothing written behind the image");
						for(q = 0; q < 3; q++)
							CHECK(!memcmp(img + q * mine, whole + q * words + per * (size_t)kfirst, 8 * mine), "image == triple loop");
						CHECK(pft_snapshot_region_ranges(path, &g, r, &ranges) == 0, "region_ranges");
						CHECK(ranges.bytes == 8 * mine, "ranges.bytes");
						CHECK(pft_snapshot_write_image(path, &ranges, mine ? img : NULL) == 0, "write_image");
					}
					free(img); free(x);
				}
				{
					pft_snapshot_ranges ranges;
					int d1, d2, d3;
					pft_snapshot_info got;
					CHECK(pft_snapshot_region_ranges(path, &one, r, &ranges) == 0 && ranges.bytes == 8 * words, "the whole range");
					CHECK(pft_snapshot_read_image(path, &ranges, back) == 0 && !memcmp(back, whole, 24 * words), "file == triple loop");
					CHECK(pft_snapshot_read_info(path, &d1, &d2, &d3, &got, NULL) == 0 && d1 == r->count[0] &&
					      d2 == r->count[1] && d3 == r->count[2] && !strcmp(got.title, info.title), "read_info");
					if(rg) CHECK(pft_snapshot_slab_ranges(path, &one, &ranges) == -4, "a restart from it is refused");
					else CHECK(pft_snapshot_slab_ranges(path, &one, &ranges) == 0, "the whole grid's region restarts");
				}
				unlink(path);
			}
			free(whole); free(back);
		}
	}
}

int main(void)
{
	char dir[] = "/tmp/pft_region_selftest_XXXXXX";
	if(!mkdtemp(dir)) { perror("mkdtemp"); return 1; }
	local_exhaustive();
	check_rules();
	images(dir);
	rmdir(dir);
	printf("pft_region_selftest: %ld checks, %ld failures\n", cases, failures);
	return failures ? 1 : 0;
}
