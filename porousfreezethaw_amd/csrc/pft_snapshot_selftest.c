/*
 * pft_snapshot_selftest.c -- a stand-alone host program over pft_io.c for runs under the host
 * sanitizers (make -C porousfreezethaw_amd snapshot-selftest: once with -fsanitize=thread, once with
 * -fsanitize=address,undefined; no GPU, no Python): the image of a padded host array against the
 * bytes pft_snapshot_write_slab writes, and the background writer -- several jobs queued from host
 * buffers into temporary files and their bytes checked, a buffer released and reused while other
 * jobs are queued, a path that cannot be opened reported by the next wait, and a shutdown with jobs
 * in flight, after which the writer starts again.  Exit status 0 when every case holds, 1 otherwise.
 */
#define _XOPEN_SOURCE 700
#include "../../include/pft_io.h"
#include "../../include/pft_comm.h"

#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

/* pft_snapshot_write's communicator (pft_comm.hip, not linked here): one rank */
pft_comm * pft_comm_current(void) { return NULL; }
int pft_comm_allreduce_max_i64(pft_comm * c, long long * v) { (void)c; (void)v; return 0; }

static int failures;
#define CHECK(cond, what) do { if(!(cond)) { printf("FAIL %s (line %d)\n", what, __LINE__); failures++; } } while(0)

enum { N1 = 7, N2 = 5, N3 = 6, JOBS = 6 };

static void fill(double * x, const pft_grid * g, int seed)
{
	const long S = (long)(g->n1 + 4) * (g->n2 + 4) * (g->n3 + 4);
	long i;
	uint64_t s = 0x9e3779b97f4a7c15ULL * (uint64_t)(seed + 1);
	for(i = 0; i < 3 * S; i++) {
		s ^= s << 13; s ^= s >> 7; s ^= s << 17;
		x[i] = (double)(int64_t)(s >> 12) * 0x1p-40 - 1000.0;
	}
}

static unsigned char * file_ranges(const char * path, const pft_snapshot_ranges * r)
{
	unsigned char * out = (unsigned char *)malloc(3 * (size_t)r->bytes);
	FILE * f = fopen(path, "rb");
	int q;
	if(!out || !f) { CHECK(0, "open for reading"); if(f) fclose(f); free(out); return NULL; }
	for(q = 0; q < 3; q++) {
		fseek(f, (long)r->off[q], SEEK_SET);
		if(fread(out + (size_t)q * r->bytes, 1, (size_t)r->bytes, f) != (size_t)r->bytes) CHECK(0, "short read");
	}
	fclose(f);
	return out;
}

int main(void)
{
	char dir[] = "/tmp/pft_snapshot_selftest_XXXXXX";
	char path[JOBS][256], bad[256];
	pft_grid g;
	pft_snapshot_info info;
	pft_snapshot_ranges r[JOBS];
	double param[PFT_PARAM_COUNT];
	double * x;
	unsigned char * img[JOBS], * want, * got;
	size_t bytes;
	long S;
	int i, rc;

	memset(&g, 0, sizeof g); memset(&info, 0, sizeof info);
	g.n1 = N1; g.n2 = N2; g.n3 = N3; g.total_n3 = N3; g.nprocs = 1;
	g.L1 = 0.03; g.L2 = 0.03; g.L3 = 0.06;
	for(i = 0; i < PFT_PARAM_COUNT; i++) param[i] = 1.0 + i;
	info.t = 36.0; info.tau = 0.5; info.final_time = 72.0; info.delta = 1e-3; info.total_snapshots = JOBS;
	pft_snapshot_title(info.title, sizeof info.title, "selftest", info.t);
	if(!mkdtemp(dir)) { perror("mkdtemp"); return 1; }
	S = (long)(N1 + 4) * (N2 + 4) * (N3 + 4);
	bytes = pft_snapshot_image_bytes(&g);
	CHECK(bytes == 24u * N1 * N2 * N3, "image bytes");
	x = (double *)malloc(sizeof(double) * 3 * (size_t)S);
	want = (unsigned char *)malloc(bytes);
	if(!x || !want) return 1;

	/* the image of a padded array is what write_slab puts into the file */
	for(i = 0; i < JOBS; i++) {
		snprintf(path[i], sizeof path[i], "%s/job%d.ncd", dir, i);
		info.snapshot = i;
		CHECK(pft_snapshot_create(path[i], &g, param, &info, i & 1 ? 2 : 1) == 0, "create");
		CHECK(pft_snapshot_slab_ranges(path[i], &g, &r[i]) == 0, "ranges");
		CHECK(r[i].bytes * 3 == bytes, "range bytes");
		img[i] = (unsigned char *)malloc(bytes);
		if(!img[i]) return 1;
	}
	fill(x, &g, 100);
	CHECK(pft_snapshot_image_host(&g, x, want) == 0, "image_host");
	CHECK(pft_snapshot_write_slab(path[0], &g, x) == 0, "write_slab");
	got = file_ranges(path[0], &r[0]);
	CHECK(got && !memcmp(got, want, bytes), "image == write_slab's bytes");
	free(got);

	/* JOBS jobs queued at once, then every file checked */
	for(i = 0; i < JOBS; i++) {
		fill(x, &g, i);
		CHECK(pft_snapshot_image_host(&g, x, img[i]) == 0, "image_host");
		CHECK(pft_snapshot_write_image_async(path[i], &r[i], img[i]) == 0, "queue");
	}
	CHECK(pft_snapshot_writer_wait() == 0, "wait");
	for(i = 0; i < JOBS; i++) {
		got = file_ranges(path[i], &r[i]);
		CHECK(got && !memcmp(got, img[i], bytes), "file holds its job's image");
		free(got);
	}
	/* read back through read_image, and into a padded array */
	CHECK(pft_snapshot_read_image(path[3], &r[3], want) == 0 && !memcmp(want, img[3], bytes), "read_image");
	{
		double * y = (double *)calloc(3 * (size_t)S, sizeof(double));
		if(!y) return 1;
		CHECK(pft_snapshot_read_slab(path[3], &g, y) == 0, "read_slab");
		CHECK(pft_snapshot_image_host(&g, y, want) == 0 && !memcmp(want, img[3], bytes), "read_slab gives the image's state");
		free(y);
	}

	/* one buffer reused: release() returns once its job is done, while other jobs are still queued */
	for(i = 0; i < 3 * JOBS; i++) {
		const int b = i % 2, f = i % JOBS;
		CHECK(pft_snapshot_writer_release(img[b]) == 0, "release");
		fill(x, &g, 1000 + i);
		CHECK(pft_snapshot_image_host(&g, x, img[b]) == 0, "image_host");
		CHECK(pft_snapshot_write_image_async(path[f], &r[f], img[b]) == 0, "queue");
	}
	CHECK(pft_snapshot_writer_wait() == 0, "wait after reuse");
	got = file_ranges(path[(3 * JOBS - 1) % JOBS], &r[(3 * JOBS - 1) % JOBS]);
	CHECK(got && !memcmp(got, img[(3 * JOBS - 1) % 2], bytes), "the last job's image is in its file");
	free(got);

	/* a path that cannot be opened: the next wait reports it with errno kept, once; the jobs
	   beside it are written */
	snprintf(bad, sizeof bad, "%s/no/such.ncd", dir);
	CHECK(pft_snapshot_write_image_async(path[2], &r[2], img[2]) == 0, "queue");
	CHECK(pft_snapshot_write_image_async(bad, &r[2], img[3]) == 0, "queue the failing job");
	CHECK(pft_snapshot_write_image_async(path[4], &r[4], img[4]) == 0, "queue");
	errno = 0;
	rc = pft_snapshot_writer_wait();
	CHECK(rc == -1 && errno == ENOENT, "the failing job is reported with its errno");
	CHECK(pft_snapshot_writer_wait() == 0, "... once");
	got = file_ranges(path[4], &r[4]);
	CHECK(got && !memcmp(got, img[4], bytes), "the job after the failing one is written");
	free(got);
	CHECK(pft_snapshot_write_image_async(NULL, &r[0], img[0]) == -2, "bad arguments");

	/* shutdown with jobs in flight: they are written first; a later job starts a new thread */
	for(i = 0; i < JOBS; i++) {
		fill(x, &g, 2000 + i);
		pft_snapshot_image_host(&g, x, img[i]);
		CHECK(pft_snapshot_write_image_async(path[i], &r[i], img[i]) == 0, "queue");
	}
	CHECK(pft_snapshot_writer_shutdown() == 0, "shutdown");
	for(i = 0; i < JOBS; i++) {
		got = file_ranges(path[i], &r[i]);
		CHECK(got && !memcmp(got, img[i], bytes), "shutdown wrote the queued jobs");
		free(got);
	}
	CHECK(pft_snapshot_writer_shutdown() == 0, "shutdown twice");
	fill(x, &g, 3000);
	pft_snapshot_image_host(&g, x, img[0]);
	CHECK(pft_snapshot_write_image_async(path[0], &r[0], img[0]) == 0, "queue after shutdown");
	CHECK(pft_snapshot_writer_release(img[0]) == 0 && pft_snapshot_writer_wait() == 0, "the writer runs again");
	got = file_ranges(path[0], &r[0]);
	CHECK(got && !memcmp(got, img[0], bytes), "the job after a shutdown is written");
	free(got);
	CHECK(pft_snapshot_writer_shutdown() == 0, "last shutdown");

	for(i = 0; i < JOBS; i++) { unlink(path[i]); free(img[i]); }
	rmdir(dir);
	free(x); free(want);
	printf(failures ? "pft_snapshot_selftest: %d failure(s)\n" : "pft_snapshot_selftest: ok\n", failures);
	return failures ? 1 : 0;
}
