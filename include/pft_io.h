/*
 * pft_io.h -- snapshot / restart datasets of the intertrack (u, p, gl) state.
 *
 * The reference writes every snapshot with the NetCDF library in its classic format
 * (intertrack.c:2331 nc_create(..., NC_CLOBBER)) and reads one back for `icond_file` /
 * `continue_series` restarts (intertrack.c:1584-1669, 2040-2069).  NetCDF is not available in
 * this image, so libpft writes the same dataset with its own NetCDF-classic writer:
 *   - dimensions n3 = total_n3, n2, n1 (interior cells, grid_IO_mode 1, :2338-2340);
 *   - coordinate variables n3, n2, n1 (double): L3*(0.5+k)/total_n3, L2*(0.5+j)/n2, L1*(0.5+i)/n1
 *     (:2441-2443), then one double variable per model variable, u, p, gl, [n3][n2][n1] (:2354);
 *   - global attributes in the reference's order (:2382-2406): L1, L2, L3, the model parameters
 *     in param_info[] order (model.c:85-137), calc_mode (int), delta, tau, t, final_time,
 *     snapshot (int), total_snapshots (int), title (text).
 * Format: CDF-1 ("classic") when the file stays below 2 GiB, CDF-2 (64-bit offsets) above it
 * (the 800^3 case), readable by any NetCDF reader.  Data are big-endian, as the format requires.
 *
 * Multi-GPU: one shared file, no gather.  pft_snapshot_create() (one rank) writes the header,
 * the coordinates and sizes the file; after a barrier every rank writes its own Z-slab planes
 * with pft_snapshot_write_slab() at their offsets.  pft_snapshot_write() does both over the
 * current pft communicator.  Host layout of x is the reference's padded layout (pft_model.h).
 * Return codes: 0 OK; -1 I/O error (errno kept); -2 bad argument; -3 not a NetCDF classic file or
 * a variable/dimension missing; -4 dimensions differ from the grid.
 */
#ifndef PFT_IO_H
#define PFT_IO_H

#include <stddef.h>

#include "pft_model.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
	double t;               /* eqSystem.t */
	double tau;             /* eqSystem.h (the next step size) */
	double final_time;
	double delta;
	int snapshot, total_snapshots;
	int calc_mode;
	char title[256];        /* "Intertrack simulation (<comment>). Time: <t>" (:1129, :2405) */
	double L1, L2, L3;      /* read back from the dataset (written from the grid) */
} pft_snapshot_info;

/* header + coordinate variables, file sized to its final length; param = PFT_PARAM_COUNT values
   in pft_model.h order (written in param_info order); version 0 = automatic, 1 = CDF-1, 2 = CDF-2 */
int pft_snapshot_create(const char * path, const pft_grid * g, const double * param,
                        const pft_snapshot_info * info, int version);
/* this slab's interior planes of u, p, gl from the host padded array x */
int pft_snapshot_write_slab(const char * path, const pft_grid * g, const double * x);
/* create (rank 0) + barrier + write_slab (every rank) over the current communicator */
int pft_snapshot_write(const char * path, const pft_grid * g, const double * param,
                       const pft_snapshot_info * info, const double * x);

/* dimensions, attributes (info) and, if param != NULL, the model parameters of a dataset */
int pft_snapshot_read_info(const char * path, int * n1, int * n2, int * total_n3,
                           pft_snapshot_info * info, double * param);
/* the attributes a continued series starts from (continue_series, intertrack.c:1650-1662):
   snapshot, total_snapshots, t, final_time, tau; -3 when one of them is missing */
int pft_snapshot_read_series(const char * path, int * snapshot, int * total_snapshots, double * t,
                             double * final_time, double * tau);
/* this slab's interior planes into the host padded array x (ghost cells untouched) */
int pft_snapshot_read_slab(const char * path, const pft_grid * g, double * x);

/* f7: the image of a slab: for q = u, p, gl in turn its n3*n1*n2 interior doubles as big-endian
   8-byte words -- exactly the bytes the slab owns in each variable of the dataset.  image_host
   builds it from the host padded array (the twin of the device's pft_slab_export_be); ranges are
   the three places of a slab's image in an existing dataset (-4: its dimensions differ from the
   grid's), write_image / read_image move an image there and back (pwrite / pread of this slab's
   planes only). */
typedef struct {
	unsigned long long off[3];   /* file offset of this slab's planes of u, p, gl */
	unsigned long long bytes;    /* per variable: 8 * n3 * n1 * n2 */
} pft_snapshot_ranges;
size_t pft_snapshot_image_bytes(const pft_grid * g);
int pft_snapshot_image_host(const pft_grid * g, const double * x_padded, void * out);
int pft_snapshot_slab_ranges(const char * path, const pft_grid * g, pft_snapshot_ranges * r);
int pft_snapshot_write_image(const char * path, const pft_snapshot_ranges * r, const void * image);
int pft_snapshot_read_image(const char * path, const pft_snapshot_ranges * r, void * image);
/* The background writer: one thread per process, started by the first job, which writes the jobs
   in the order they were queued.  It calls no HIP function and only reads the image, which must
   stay unchanged until the job is done: writer_release(image) returns once no queued or running
   job reads that buffer (before it is overwritten or freed); writer_wait() returns once every job
   is done, with the first error since the previous wait (-1 and errno kept; 0 none);
   writer_shutdown() writes what is queued and joins the thread (a later job starts a new one). */
int pft_snapshot_write_image_async(const char * path, const pft_snapshot_ranges * r, const void * image);
int pft_snapshot_writer_release(const void * image);
int pft_snapshot_writer_wait(void);
int pft_snapshot_writer_shutdown(void);

/* f11: a *region* of the grid -- per axis the global interior indices start + m*stride, m = 0 ..
   count-1 ([0] = i of n1, [1] = j of n2, [2] = k of total_n3; every stride and count at least 1,
   the last index inside the grid) -- and its dataset: a snapshot dataset of the selected cells
   alone.  Dimensions n3, n2, n1 = the counts; the coordinate variables are the full dataset's
   entries at the selected indices, bit for bit; the global attributes are a full dataset's, in
   its order, followed by three int[3] attributes region_start, region_count, region_stride in
   (i, j, k) order; CDF-1 / CDF-2 by the rule of pft_snapshot_create.  A full dataset is unchanged.
     region_check   0, or -2 for a region that breaks a rule above;
     region_local   this slab's share of the region's k axis: *kfirst the index within that axis
                    of the first selected plane the slab owns, *kcount how many it owns (0: none;
                    then *kfirst is where they would lie and *klocal is 0), *klocal the slab-local
                    plane (0-based) of the first one;
     region_image_bytes / region_image_host   the region image of a slab, the host twin of
                    pft_slab_export_region_be: for q = u, p, gl in turn its kcount * count[1] *
                    count[0] selected doubles as big-endian words, [k][j][i] with i fastest;
     create_region / region_ranges   the dataset's header and coordinates, and the three places
                    of this slab's region image in it (bytes 0 for a slab that owns none; -4 when
                    the dataset's dimensions are not the region's counts).
   write_image, write_image_async and read_image take these ranges as they take a slab's; ranges of
   0 bytes move nothing and succeed.  As a restart a region dataset is refused by its dimensions
   (-4), unless it selects the whole grid. */
typedef struct { int start[3], count[3], stride[3]; } pft_region;   /* [0] = i (n1), [1] = j (n2), [2] = k (total_n3) */
int pft_region_check(const pft_grid * g, const pft_region * r);
int pft_region_local(const pft_grid * g, const pft_region * r, int * kfirst, int * kcount, int * klocal);
size_t pft_region_image_bytes(const pft_grid * g, const pft_region * r);
int pft_region_image_host(const pft_grid * g, const pft_region * r, const double * x_padded, void * out);
int pft_snapshot_create_region(const char * path, const pft_grid * g, const pft_region * r, const double * param,
                               const pft_snapshot_info * info, int version);
int pft_snapshot_region_ranges(const char * path, const pft_grid * g, const pft_region * r, pft_snapshot_ranges * ranges);
/* the host path, as pft_snapshot_write: create_region (rank 0) + barrier + every rank's region
   image of the host padded array x into its ranges, over the current communicator */
int pft_snapshot_write_region(const char * path, const pft_grid * g, const pft_region * r, const double * param,
                              const pft_snapshot_info * info, const double * x, int version);

/* the title the reference writes (:1129, :2405): "Intertrack simulation (%s). Time: %g" */
int pft_snapshot_title(char * buf, int size, const char * comment, double t);

#ifdef __cplusplus
}
#endif
#endif
