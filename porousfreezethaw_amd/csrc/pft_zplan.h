// pft_zplan.h -- the z-chunk plan of a stage or pair launch: the one place that knows which
// workgroup runs which planes.  Plain host code (no HIP, no slab): run_stage and run_pair fill
// their kernel arguments from pft_zplan_make, the kernels find their planes with pft_zplan_chunk and
// pft_zplan_planes, and tests/native/zplan_check.cpp walks every workgroup of every plan on the CPU.
#ifndef PFT_ZPLAN_H
#define PFT_ZPLAN_H

#if defined(__HIPCC__)
#define PFT_ZP_HD __host__ __device__ __forceinline__
#else
#define PFT_ZP_HD static inline
#endif

// the k_begin codes of include/pft_hip.h, restated so that this header stands alone (pft_kernels.hip
// checks that they agree)
enum { PFT_ZP_BOUNDARY = -2, PFT_ZP_BOUNDARY2 = -3, PFT_ZP_INLINE = -4, PFT_ZP_ENDS_FIRST = -5 };

// bijective on [0, n): the blocks the dispatcher deals to one XCD (b % 8 equal) get consecutive ids
PFT_ZP_HD int xcd_remap(int b, int n)
{
  const int q = n >> 3, r = n & 7, x = b & 7, l = b >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + l;
}

// planes per z-chunk: a CU runs `occ` workgroups at a time; a chunk count with w = ceil(workgroups /
// CUs) workgroups per CU costs (planes per chunk + the two planes a chunk re-reads) times
//   - occ <= 2: ceil(w / occ) rounds -- a partial last round runs a CU at half its waves and the
//     HBM-bound stages stall;
//   - occ >= 3: max(1, w / occ) -- retiring workgroups are refilled at once, and the extra
//     workgroups help the arithmetic-heavy stages hide latency.
// The cheapest count wins (more chunks only when 5% cheaper).  min_nch >= 3: at least that many
// chunks, the first and the last of two planes or more (ends-first).  ncu: the compute stream's
// CUs.  nplanes >= 1.
static inline int pft_zplan_kz(int occ, long ntile, int nplanes, int min_nch, int ncu)
{
  int best_nch = 1;
  double best_cost = -1.0;
  if (min_nch > nplanes) min_nch = nplanes;
  for (int nch = min_nch; nch <= nplanes; ++nch) {
    const int k = (nplanes + nch - 1) / nch;
    if (nch > min_nch && k == (nplanes + nch - 2) / (nch - 1)) continue;   // same kz as nch - 1
    if ((nplanes + k - 1) / k < min_nch) continue;
    if (min_nch >= 3 && (k < 2 || nplanes - ((nplanes + k - 1) / k - 1) * k < 2)) continue;   // edge chunks >= 2 planes
    const long nb = ntile * ((nplanes + k - 1) / k);
    const long per_cu = (nb + ncu - 1) / ncu;
    const double rounds = occ <= 2 ? (double)((per_cu + occ - 1) / occ) : (per_cu > occ ? (double)per_cu / occ : 1.0);
    const double cost = rounds * (k + 2);
    if (best_cost < 0.0 || cost < 0.95 * best_cost) { best_cost = cost; best_nch = nch; }
  }
  if (best_cost < 0.0) best_nch = nplanes > 1 ? nplanes : 1;
  return (nplanes + best_nch - 1) / best_nch;
}

// a launch's plan: the StageArgs / PairArgs fields of the same names, and what the launcher's tail
// needs to know about it
typedef struct pft_zplan {
  // chunk c runs planes [k_begin + c kz, + kspan) below k_end.  The grid's first nbw workgroups (0:
  // none) lead: bends 0, the two planes at each end (chunk 0: planes 0, 1; chunk 1: n3-2, n3-1), the
  // other nint workgroups the chunks of [k_begin, k_end); bends 1, the first and the last chunk of
  // every tile column, the others chunks c0 ..
  int k_begin, k_end, kz, kspan, nchunk, nbw, bends, c0, nint;
  int bnd;        // a boundary launch (PFT_K_BOUNDARY: depth 1, PFT_K_BOUNDARY2: depth 2)
  int inl;        // an inline boundary: the first nbw workgroups produce the exchanged planes
  int fallback;   // PFT_K_ENDS_FIRST served as PFT_K_INLINE (the chunks cannot hold the end planes)
} pft_zplan;

// what a plan asks of its launcher
typedef struct pft_zplan_in {
  int k_begin, k_end;   // a range code in k_begin, or planes [k_begin, k_end) (-1/-1: all)
  int n3, ntile;
  int kz;               // forced planes per chunk, 0: the cost model
  int occ, ncu;         // the cost model's: resident workgroups per CU, the compute stream's CUs
  int depths;           // boundary launches served: bit 0 depth 1, bit 1 depth 2
  int can_inline;       // the launcher can serve PFT_K_INLINE / PFT_K_ENDS_FIRST now
  // the cost model behind the launcher's memo `memo` (null: pft_zplan_kz itself)
  int (*kz_of)(void* memo, int occ, long ntile, int nplanes, int min_nch, int ncu);
  void* memo;
} pft_zplan_in;

static inline int pft_zplan_auto_kz(const pft_zplan_in* in, int nplanes, int min_nch)
{
  return in->kz_of ? in->kz_of(in->memo, in->occ, in->ntile, nplanes, min_nch, in->ncu)
                   : pft_zplan_kz(in->occ, in->ntile, nplanes, min_nch, in->ncu);
}

// 1: launch p->nbw + p->nint workgroups; 0: an empty range, nothing to launch; -2: a request the
// launcher cannot serve
static inline int pft_zplan_make(pft_zplan* p, const pft_zplan_in* in)
{
  const int n3 = in->n3, ntile = in->ntile;
  const pft_zplan zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  *p = zero;
  // a boundary launch: the `depth` planes at each end in ONE launch, two chunks n3 - depth planes
  // apart (what the z-neighbours need first)
  const int bnd = in->k_begin == PFT_ZP_BOUNDARY || in->k_begin == PFT_ZP_BOUNDARY2;
  const int depth = in->k_begin == PFT_ZP_BOUNDARY2 ? 2 : 1;
  // inline boundary: the whole slab, the first and last chunk of every tile column leading (ends),
  // or two-plane chunks at each end leading the interior [2, n3 - 2)
  int ends = in->k_begin == PFT_ZP_ENDS_FIRST;
  const int inl = in->k_begin == PFT_ZP_INLINE || ends;
  if (bnd && !(in->depths & depth)) return -2;
  if (inl && (!in->can_inline || n3 < 5)) return -2;
  if (ends) {
    // the first and the last chunk must hold the two planes at each end (kz >= 2, a last chunk of
    // two planes or more) and leave a chunk between them (at least three chunks, so that the ends
    // of a column are done while the others still run: the exchange's copies go beside them);
    // otherwise the two-plane boundary chunks
    const int kz = in->kz > 0 ? in->kz : pft_zplan_auto_kz(in, n3, 3);
    const int nch = (n3 + kz - 1) / kz;
    if (kz < 2 || nch < 3 || n3 - (nch - 1) * kz < 2) {
      ends = 0;
      p->fallback = 1;
    }
  }
  int kb = in->k_begin, ke = in->k_end;
  if (inl) {
    kb = ends ? 0 : 2;
    ke = ends ? n3 : n3 - 2;
  }
  if (bnd || kb < 0) kb = 0;
  if (bnd || ke < 0 || ke > n3) ke = n3;
  if (ke <= kb) return 0;   // (the cost model divides by the plane count)
  p->k_begin = kb;
  p->k_end = ke;
  p->bnd = bnd;
  p->inl = inl;
  if (bnd) {
    p->kz = n3 - depth > 1 ? n3 - depth : 1;
    p->kspan = depth;
    p->nchunk = n3 > depth ? 2 : 1;
  } else {
    p->kz = in->kz > 0 ? in->kz : pft_zplan_auto_kz(in, ke - kb, ends ? 3 : 1);
    p->kspan = p->kz;
    p->nchunk = (ke - kb + p->kz - 1) / p->kz;
  }
  p->nint = ntile * p->nchunk;
  if (ends) {
    const int nb = p->nchunk < 2 ? p->nchunk : 2;
    p->nbw = nb * ntile;
    p->bends = 1;
    p->c0 = 1;
    p->nint = (p->nchunk - nb) * ntile;
  } else if (inl) {
    p->nbw = 2 * ntile;
  }
  return 1;
}

// Workgroup b of a launch -> its tile and z-chunk, from the plan fields of its kernel arguments (by
// value: the kernels' argument structs stay in the kernarg segment).  A launch without leading
// workgroups (nbw == 0: merson_stage):
PFT_ZP_HD void pft_zplan_chunk_flat(int b, int ntile, int nchunk, int* tile, int* chunk)
{
  const int lin = xcd_remap(b, ntile * nchunk);
  *tile = lin % ntile;
  *chunk = lin / ntile;
}

// ... and any launch.  Inline boundary: the leading workgroups (bw; dispatched first) produce the
// planes the exchange sends, bshort: as a two-plane boundary chunk (PFT_K_INLINE)
PFT_ZP_HD void pft_zplan_chunk(int b, int ntile, int nchunk, int nbw, int bends, int c0, int nint, int* tile,
                               int* chunk, bool* bw, bool* bshort)
{
  *bw = b < nbw;
  const int lin = *bw ? xcd_remap(b, nbw) : xcd_remap(b - nbw, nint);
  *tile = lin % ntile;
  const int cq = lin / ntile;
  *chunk = *bw ? (bends ? (cq ? nchunk - 1 : 0) : cq) : c0 + cq;
  *bshort = *bw && !bends;
}

// the planes [kb, ke) of a chunk
PFT_ZP_HD void pft_zplan_planes(int chunk, bool bshort, int n3, int k_begin, int k_end, int kz, int kspan, int* kb,
                                int* ke)
{
  *kb = bshort ? chunk * (n3 - 2) : k_begin + chunk * kz;
  *ke = bshort ? *kb + 2 : (*kb + kspan < k_end ? *kb + kspan : k_end);
}

#endif
