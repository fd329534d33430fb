// pft_snap.hip -- device-side snapshots: snap_kernel, export, import and the pinned image (f7);
// region_kernel and the region image (f11).
#include "pft_slab.h"

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------
// f7: the snapshot image of a state (pft_io.h) -- for q = u, p, gl in turn the slab's n3*n1*n2
// interior doubles as big-endian 8-byte words, the bytes the slab owns in each variable of the
// dataset.  In the slab's layout a field's interior is one contiguous run from plane 1, i fastest
// (what diag_kernel streams), which is the [n3][n2][n1] order of the dataset's variable, so the
// export is a byte swap of three runs and the import its inverse.  One flat streaming kernel for
// both directions, blockIdx.y the field: the run is taken in 16-byte pairs from the first 16-byte
// boundary of the slab's side, PFT_SNAP_NV pairs per lane and iteration, all loaded before the
// first is used; the pair's words are swapped as integers (a pure bit move: NaN payloads, -0.0 and
// subnormals survive) and stored as one 16-byte store, or as two 8-byte stores when the image's
// side of that field is only 8-byte aligned (an odd run length puts the second field there).  The
// element before the first pair (an odd `head`) and the one after the last (an odd rest) are moved
// by one lane.  No LDS; the export has no atomic at all.  Ghost and far ghost planes are never
// touched.  The import writes X and XN, as the device IC does, and reports whether a gl value is
// -0.0 or NaN (pft_slab_set_gl_keep): a ballot per wave and one integer atomic.

#define PFT_SNAP_BLOCK 256
#define PFT_SNAP_NV 4
#define PFT_SNAP_WG_PAIRS (PFT_SNAP_BLOCK * PFT_SNAP_NV)

typedef unsigned long long snap_u64;

__device__ __forceinline__ bool snap_gl_unclean(snap_u64 v)
{
  // -0.0, or NaN (exponent all ones, mantissa non-zero)
  return v == 0x8000000000000000ULL || (v & 0x7fffffffffffffffULL) > 0x7ff0000000000000ULL;
}

// one iteration of a workgroup: PFT_SNAP_NV pairs per lane from pair p0 on.  FULL: all of them lie
// in the run, and the code is straight-line -- every load is issued before the first swap; else a
// pair past the run's end loads the last pair instead and is not stored.  S16 / D16: that side
// takes 16-byte accesses
template <bool IMPORT, bool S16, bool D16, bool FULL>
__device__ __forceinline__ bool snap_iter(const snap_u64* __restrict__ sp, snap_u64* __restrict__ dp,
                                          snap_u64* __restrict__ dp2, long p0, long m, bool scan)
{
  bool bad = false;
  snap_u64 a[PFT_SNAP_NV], b[PFT_SNAP_NV];
#pragma unroll
  for (int i = 0; i < PFT_SNAP_NV; ++i) {
    const long p = p0 + (long)i * PFT_SNAP_BLOCK, pc = (FULL || p < m) ? p : m - 1;
    if (S16) {
      const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(sp + 2 * pc);
      a[i] = v.x;
      b[i] = v.y;
    } else {
      a[i] = sp[2 * pc];
      b[i] = sp[2 * pc + 1];
    }
  }
#pragma unroll
  for (int i = 0; i < PFT_SNAP_NV; ++i) {
    const long p = p0 + (long)i * PFT_SNAP_BLOCK;
    if (FULL || p < m) {
      const snap_u64 x = __builtin_bswap64(a[i]), y = __builtin_bswap64(b[i]);
      if (IMPORT && scan) bad = bad || snap_gl_unclean(x) || snap_gl_unclean(y);
      if (D16) {
        ulonglong2 v;
        v.x = x;
        v.y = y;
        *reinterpret_cast<ulonglong2*>(dp + 2 * p) = v;
        if (IMPORT) *reinterpret_cast<ulonglong2*>(dp2 + 2 * p) = v;
      } else {
        dp[2 * p] = x;
        dp[2 * p + 1] = y;
        if (IMPORT) {
          dp2[2 * p] = x;
          dp2[2 * p + 1] = y;
        }
      }
    }
  }
  return bad;
}

// pairs [0, m) of sp -> dp (and dp2)
template <bool IMPORT, bool S16, bool D16>
__device__ __forceinline__ bool snap_run(const snap_u64* __restrict__ sp, snap_u64* __restrict__ dp,
                                         snap_u64* __restrict__ dp2, long m, bool scan)
{
  bool bad = false;
  for (long c = blockIdx.x; c * PFT_SNAP_WG_PAIRS < m; c += gridDim.x) {
    const long p0 = c * PFT_SNAP_WG_PAIRS + threadIdx.x;
    if ((c + 1) * PFT_SNAP_WG_PAIRS <= m)
      bad = snap_iter<IMPORT, S16, D16, true>(sp, dp, dp2, p0, m, scan) || bad;
    else
      bad = snap_iter<IMPORT, S16, D16, false>(sp, dp, dp2, p0, m, scan) || bad;
  }
  return bad;
}

// src / dst: word 0 of field 0's run on either side, strides in words; n words per field.  IMPORT:
// dst2 is the second state buffer (the same alignment as dst: checked by the host)
template <bool IMPORT>
__global__ __launch_bounds__(PFT_SNAP_BLOCK) void snap_kernel(const snap_u64* __restrict__ src, long src_stride,
                                                              snap_u64* __restrict__ dst, snap_u64* __restrict__ dst2,
                                                              long dst_stride, long n, unsigned int* __restrict__ unclean)
{
  const int q = blockIdx.y;
  const snap_u64* sp = src + (long)q * src_stride;
  snap_u64* dp = dst + (long)q * dst_stride;
  snap_u64* dp2 = IMPORT ? dst2 + (long)q * dst_stride : nullptr;
  const bool scan = IMPORT && q == 2;
  // the slab's side decides where the pairs begin; the image's side follows
  const uintptr_t slab_side = IMPORT ? (uintptr_t)dp : (uintptr_t)sp;
  const long head = (n > 0 && ((slab_side >> 3) & 1)) ? 1 : 0;
  const long m = (n - head) / 2;
  const bool tail = ((n - head) & 1) != 0;
  const uintptr_t image_side = IMPORT ? (uintptr_t)(sp + head) : (uintptr_t)(dp + head);
  bool bad;
  if ((image_side & 15) == 0)
    bad = snap_run<IMPORT, true, true>(sp + head, dp + head, IMPORT ? dp2 + head : nullptr, m, scan);
  else if (IMPORT)
    bad = snap_run<IMPORT, false, true>(sp + head, dp + head, dp2 + head, m, scan);
  else
    bad = snap_run<IMPORT, true, false>(sp + head, dp + head, nullptr, m, scan);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // the run's ends, element-wise
    if (head) {
      const snap_u64 x = __builtin_bswap64(sp[0]);
      if (scan) bad = bad || snap_gl_unclean(x);
      dp[0] = x;
      if (IMPORT) dp2[0] = x;
    }
    if (tail) {
      const snap_u64 x = __builtin_bswap64(sp[n - 1]);
      if (scan) bad = bad || snap_gl_unclean(x);
      dp[n - 1] = x;
      if (IMPORT) dp2[n - 1] = x;
    }
  }
  if (IMPORT) {
    const unsigned long long any = __ballot(bad);
    if (scan && any && (threadIdx.x & 63) == 0) atomicOr(unclean, 1u);
  }
}

static unsigned snap_blocks(const pft_slab* s, long n)
{
  // all resident at once (8 workgroups per CU), each a whole number of iterations
  const long cap = 8L * (s->n_cu > 0 ? s->n_cu : 256);
  long wgs = (n / 2 + PFT_SNAP_WG_PAIRS - 1) / PFT_SNAP_WG_PAIRS;
  if (wgs < 1) wgs = 1;
  return (unsigned)(wgs > cap ? cap : wgs);
}

// the export kernel of buffer `buf` into dst, enqueued on the compute stream (no wait)
static int snap_export_enqueue(pft_slab* s, int buf, void* dst)
{
  const long n = (long)s->d.n3 * s->plane;
  const snap_u64* src = reinterpret_cast<const snap_u64*>(s->buf[buf] + s->plane);   // plane 1: the interior
  if (s->snap_timing) HIPCHK(hipEventRecord(s->ev_snap[0], s->stream));
  snap_kernel<false><<<dim3(snap_blocks(s, n), 3), PFT_SNAP_BLOCK, 0, s->stream>>>(src, s->fs, (snap_u64*)dst, nullptr, n, n,
                                                                                   nullptr);
  HIPCHK(hipGetLastError());
  if (s->snap_timing) HIPCHK(hipEventRecord(s->ev_snap[1], s->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------
// f11: the region image (pft_io.h) -- the cells start + m*stride of a box, per field a dense
// [c3][c2][c1] block of big-endian words.  One flat kernel, blockIdx.y the field: a lane moves one
// word per trip of a grid-stride loop -- an 8-byte load from the strided box, the integer byte swap
// of snap_kernel, an 8-byte store at the flat output index -- so the stores are dense and coalesced
// for every region and the loads are coalesced when stride[0] == 1.  No LDS, no atomic; only
// interior planes are addressed (plane 1 + klocal + k'*s3 of the buffer's indexing).
// The split of the flat index into (k', j', i'): a lane divides once, before the loop.  Every trip
// advances all lanes by the same number of words, gridDim.x * PFT_SNAP_BLOCK, whose own split
// (dk, dj, di) is wave-uniform and computed once; the lane adds it digit by digit with one carry
// each (i' + di < 2 c1, j' + dj + 1 <= 2 c2 - 1), so the loop holds no division whatever the row
// length -- a row of one word (a y-z section) walks as cheaply as a row of 200.

struct RegionGeom {
  long plane, n1;             // words per plane and per row of the slab
  long n;                     // words per field of the image: c1 * c2 * c3
  int i0, j0, k0;             // first selected cell; k0 slab-local (interior plane, 0-based)
  int s1, s2, s3;
  int c1, c2;
};

__global__ __launch_bounds__(PFT_SNAP_BLOCK) void region_kernel(const snap_u64* __restrict__ src, long src_stride,
                                                                snap_u64* __restrict__ dst, RegionGeom g)
{
  const snap_u64* sp = src + (long)blockIdx.y * src_stride;   // plane 0 of the field: the ghost plane
  snap_u64* dp = dst + (long)blockIdx.y * g.n;
  const long step = (long)gridDim.x * PFT_SNAP_BLOCK;
  const long row = g.c1, slice = (long)g.c1 * g.c2;
  // the step's split: uniform
  const long dk = step / slice, srem = step - dk * slice;
  const int dj = (int)(srem / row), di = (int)(srem - (long)dj * row);
  // the lane's split: once
  long o = (long)blockIdx.x * PFT_SNAP_BLOCK + threadIdx.x;
  long k = o / slice;
  const long orem = o - k * slice;
  int j = (int)(orem / row), i = (int)(orem - (long)j * row);
  for (; o < g.n; o += step) {
    const long at = g.plane * (1 + g.k0 + k * g.s3) + (long)(g.j0 + j * g.s2) * g.n1 + g.i0 + (long)i * g.s1;
    dp[o] = __builtin_bswap64(sp[at]);
    i += di;
    const int ci = i >= g.c1;
    i -= ci ? g.c1 : 0;
    j += dj + ci;
    const int cj = j >= g.c2;
    j -= cj ? g.c2 : 0;
    k += dk + cj;
  }
}

// 0: r is a region of the slab's interior (count[2] == 0 allowed: nothing to move)
static int region_local_ok(const pft_slab* s, const pft_region* r)
{
  const int n[3] = {s->d.n1, s->d.n2, s->d.n3};
  for (int a = 0; a < 3; ++a) {
    if (r->start[a] < 0 || r->stride[a] < 1 || r->count[a] < (a == 2 ? 0 : 1)) return -2;
    if (r->count[a] > 0 && r->start[a] + (long)(r->count[a] - 1) * r->stride[a] >= n[a]) return -2;
  }
  return 0;
}

static bool region_is_interior(const pft_slab* s, const pft_region* r)
{
  return r->start[0] == 0 && r->start[1] == 0 && r->start[2] == 0 && r->stride[0] == 1 && r->stride[1] == 1 &&
         r->stride[2] == 1 && r->count[0] == s->d.n1 && r->count[1] == s->d.n2 && r->count[2] == s->d.n3;
}

// the region kernel of buffer `buf` into dst, enqueued on the compute stream (no wait); the slab's
// whole interior at stride 1 is the f7 image: that export, with its 16-byte accesses
static int region_export_enqueue(pft_slab* s, int buf, const pft_region* r, void* dst)
{
  if (region_is_interior(s, r)) return snap_export_enqueue(s, buf, dst);
  RegionGeom g;
  g.plane = s->plane;
  g.n1 = s->d.n1;
  g.n = (long)r->count[0] * r->count[1] * r->count[2];
  g.i0 = r->start[0], g.j0 = r->start[1], g.k0 = r->start[2];
  g.s1 = r->stride[0], g.s2 = r->stride[1], g.s3 = r->stride[2];
  g.c1 = r->count[0], g.c2 = r->count[1];
  // all resident at once, as snap_blocks; PFT_REGION_WGS caps it further (tests: several trips)
  const long cap = s->region_wgs > 0 ? s->region_wgs : 8L * (s->n_cu > 0 ? s->n_cu : 256);
  long wgs = (g.n + PFT_SNAP_BLOCK - 1) / PFT_SNAP_BLOCK;
  if (wgs > cap) wgs = cap;
  if (s->snap_timing) HIPCHK(hipEventRecord(s->ev_snap[0], s->stream));
  if (g.n > 0) {
    region_kernel<<<dim3((unsigned)wgs, 3), PFT_SNAP_BLOCK, 0, s->stream>>>(reinterpret_cast<const snap_u64*>(s->buf[buf]), s->fs,
                                                                           (snap_u64*)dst, g);
    HIPCHK(hipGetLastError());
  }
  if (s->snap_timing) HIPCHK(hipEventRecord(s->ev_snap[1], s->stream));
  return 0;
}

static int snap_ensure_host(pft_slab* s)
{
  if (s->snap_host) return 0;
  const size_t bytes = 3 * sizeof(double) * (size_t)s->d.n3 * (size_t)s->plane;
  HIPCHK(hipHostMalloc(&s->snap_host, bytes, hipHostMallocMapped));
  const hipError_t e = hipHostGetDevicePointer(&s->snap_host_dev, s->snap_host, 0);
  if (e != hipSuccess) {
    (void)hipHostFree(s->snap_host);
    s->snap_host = s->snap_host_dev = nullptr;
    return fail(e, "hipHostGetDevicePointer (snapshot image)");
  }
  return 0;
}

extern "C" {

size_t pft_slab_image_bytes(const pft_slab* s)
{
  return s ? 3 * sizeof(double) * (size_t)s->d.n3 * (size_t)s->plane : 0;
}

int pft_slab_export_be(pft_slab* s, int buf, void* dst)
{
  if (!s || !dst || buf < 0 || buf >= PFT_BUF_COUNT || ((uintptr_t)dst & 7)) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_export_be");
  const int rc = snap_export_enqueue(s, buf, dst);
  if (rc) return rc;
  return slab_wait(s, nullptr, "pft_slab_export_be");
}

int pft_slab_import_be(pft_slab* s, const void* src, int* gl_unclean)
{
  if (!s || !src || ((uintptr_t)src & 7)) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_import_be");
  const long n = (long)s->d.n3 * s->plane;
  snap_u64* x = reinterpret_cast<snap_u64*>(s->buf[PFT_BUF_X] + s->plane);
  snap_u64* xn = reinterpret_cast<snap_u64*>(s->buf[PFT_BUF_XN] + s->plane);
  if ((((uintptr_t)x ^ (uintptr_t)xn) & 15) != 0) return -2;   // (every buffer is allocated alike)
  // X and XN change: the caller re-establishes gl_keep from *gl_unclean, as after a device IC
  s->gl_keep = 0;
  unsigned int* flag = reinterpret_cast<unsigned int*>(s->scratch + 4);   // (words 0, 1: the error norm's)
  HIPCHK(hipMemsetAsync(flag, 0, sizeof(unsigned int), s->stream));
  snap_kernel<true><<<dim3(snap_blocks(s, n), 3), PFT_SNAP_BLOCK, 0, s->stream>>>((const snap_u64*)src, n, x, xn, s->fs, n, flag);
  HIPCHK(hipGetLastError());
  unsigned int* hflag = reinterpret_cast<unsigned int*>(s->host_scratch + 4);
  HIPCHK(hipMemcpyAsync(hflag, flag, sizeof(unsigned int), hipMemcpyDeviceToHost, s->stream));
  const int rc = slab_wait(s, nullptr, "pft_slab_import_be");
  if (rc) return rc;
  if (gl_unclean) *gl_unclean = *hflag ? 1 : 0;
  return 0;
}

int pft_slab_image(pft_slab* s, void** host, void** dev)
{
  if (!s) return -2;
  const int rc = snap_ensure_host(s);
  if (rc) return rc;
  if (host) *host = s->snap_host;
  if (dev) *dev = s->snap_host_dev;
  return 0;
}

int pft_slab_snapshot_export(pft_slab* s, int buf, int link, void** image)
{
  if (!s || !image || buf < 0 || buf >= PFT_BUF_COUNT || link < 0 || link > 1) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_snapshot_export");
  int rc = snap_ensure_host(s);
  if (rc) return rc;
  // a job of the background writer may still read the buffer's previous image
  (void)pft_snapshot_writer_release(s->snap_host);
  if (link == PFT_SNAP_LINK_DIRECT) {
    if ((rc = snap_export_enqueue(s, buf, s->snap_host_dev))) return rc;
  } else {
    const size_t bytes = pft_slab_image_bytes(s);
    if (!s->snap_stage) HIPCHK(hipMalloc(&s->snap_stage, bytes));
    if ((rc = snap_export_enqueue(s, buf, s->snap_stage))) return rc;
    HIPCHK(hipMemcpyAsync(s->snap_host, s->snap_stage, bytes, hipMemcpyDeviceToHost, s->stream));
  }
  if ((rc = slab_wait(s, nullptr, "pft_slab_snapshot_export"))) return rc;
  *image = s->snap_host;
  return 0;
}

size_t pft_slab_region_image_bytes(const pft_region* r)
{
  return r ? 3 * sizeof(double) * (size_t)r->count[0] * (size_t)r->count[1] * (size_t)r->count[2] : 0;
}

int pft_slab_export_region_be(pft_slab* s, int buf, const pft_region* r, void* dst)
{
  if (!s || !r || !dst || buf < 0 || buf >= PFT_BUF_COUNT || ((uintptr_t)dst & 7) || region_local_ok(s, r)) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_export_region_be");
  const int rc = region_export_enqueue(s, buf, r, dst);
  if (rc) return rc;
  return slab_wait(s, nullptr, "pft_slab_export_region_be");
}

int pft_slab_region_export(pft_slab* s, int buf, const pft_region* r, int link, void** image)
{
  if (!s || !r || !image || buf < 0 || buf >= PFT_BUF_COUNT || link < 0 || link > 1 || region_local_ok(s, r)) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_region_export");
  int rc = snap_ensure_host(s);
  if (rc) return rc;
  // a job of the background writer may still read the buffer's previous image
  (void)pft_snapshot_writer_release(s->snap_host);
  const size_t bytes = pft_slab_region_image_bytes(r);   // at most the full image's: the box lies in the interior
  if (link == PFT_SNAP_LINK_DIRECT) {
    if ((rc = region_export_enqueue(s, buf, r, s->snap_host_dev))) return rc;
  } else {
    if (!s->snap_stage) HIPCHK(hipMalloc(&s->snap_stage, pft_slab_image_bytes(s)));
    if ((rc = region_export_enqueue(s, buf, r, s->snap_stage))) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(s->snap_host, s->snap_stage, bytes, hipMemcpyDeviceToHost, s->stream));
  }
  if ((rc = slab_wait(s, nullptr, "pft_slab_region_export"))) return rc;
  *image = s->snap_host;
  return 0;
}

int pft_slab_snapshot_timing(pft_slab* s, int on) { return slab_timing_set(s, &pft_slab::snap_timing, &pft_slab::ev_snap, on); }

int pft_slab_snapshot_last_ms(pft_slab* s, double* ms) { return slab_timing_ms(s, &pft_slab::snap_timing, &pft_slab::ev_snap, ms); }

}  // extern "C"
