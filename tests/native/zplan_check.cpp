// The z-chunk plan of a stage or pair launch (porousfreezethaw_amd/csrc/pft_zplan.h), checked on the
// CPU: for every plan of the enumeration below, every workgroup index is walked through the decode
// the kernels use (xcd_remap, pft_zplan_chunk, pft_zplan_planes), and
//   (i)   every (tile, plane) of the requested range is run by exactly one workgroup, none outside;
//   (ii)  under PFT_K_INLINE the first nbw workgroups run exactly planes 0, 1, n3-2, n3-1 of every
//         tile, the rest [2, n3-2);
//   (iii) under PFT_K_ENDS_FIRST without fallback the first nbw workgroups are chunk 0 and chunk
//         nchunk-1 of every tile, each of two planes or more;
//   (iv)  under PFT_K_ENDS_FIRST with fallback the plan equals PFT_K_INLINE's;
//   (v)   nbw + nint is the grid (tiles x chunks) and no chunk is empty;
//   (vi)  the cost model gives the values the loop it was moved from gave (KZ_TABLE).
// One known exception to (i), today's rule and kept: a two-plane boundary launch (PFT_K_BOUNDARY2) of
// a three-plane slab runs planes [0, 2) and [1, 3), plane 1 twice (the same values); the solver asks
// for that launch from five planes on.
// Stand-alone: includes nothing of the project but that header.  Prints the plans checked; exit
// status 1 with a message at the first failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../porousfreezethaw_amd/csrc/pft_zplan.h"

// the plan fields of StageArgs / PairArgs
struct Args {
  int n3, ntile, k_begin, k_end, kz, kspan, nchunk, nbw, bends, c0, nint;
};

struct Case {
  int code, k_end, n3, ntile, kz, occ, ncu, depths;
};

static long n_plans = 0, n_wg = 0;

[[noreturn]] static void fail(const Case& c, const char* what, int b = -1)
{
  fprintf(stderr, "zplan_check: %s (k_begin %d k_end %d n3 %d ntile %d kz %d occ %d ncu %d depths %d, workgroup %d)\n",
          what, c.code, c.k_end, c.n3, c.ntile, c.kz, c.occ, c.ncu, c.depths, b);
  exit(1);
}

static int make(const Case& c, pft_zplan* p)
{
  const pft_zplan_in in = {c.code, c.k_end, c.n3, c.ntile, c.kz, c.occ, c.ncu, c.depths, 1, nullptr, nullptr};
  return pft_zplan_make(p, &in);
}

// per (tile, first plane): the end of the chunk that starts there, 0: none (all 0 between plans)
static std::vector<int> nxt;
static std::vector<size_t> touched;

static void check(const Case& c)
{
  pft_zplan p;
  const int rc = make(c, &p), n3 = c.n3, nt = c.ntile;
  const bool bnd = c.code == PFT_ZP_BOUNDARY || c.code == PFT_ZP_BOUNDARY2;
  const int depth = c.code == PFT_ZP_BOUNDARY2 ? 2 : 1;
  const bool inl = c.code == PFT_ZP_INLINE || c.code == PFT_ZP_ENDS_FIRST;
  // the requested planes: one range, or the two ends
  int r0[2] = {c.code < 0 ? 0 : c.code, 0}, r1[2] = {c.k_end < 0 || c.k_end > n3 ? n3 : c.k_end, 0}, nr = 1;
  if (bnd || inl) {
    r0[0] = 0;
    r1[0] = n3;
  }
  if (bnd && n3 > 2 * depth) {
    r1[0] = depth;
    r0[1] = n3 - depth;
    r1[1] = n3;
    nr = 2;
  }
  const bool overlap = bnd && depth == 2 && n3 == 3;   // the known exception
  if (bnd && !(c.depths & depth)) {
    if (rc != -2) fail(c, "a boundary depth the launcher does not serve was planned");
    return;
  }
  if (inl && n3 < 5) {
    if (rc != -2) fail(c, "an inline boundary on fewer than five planes was planned");
    return;
  }
  if (r1[0] <= r0[0]) {
    if (rc != 0) fail(c, "an empty range was planned");
    return;
  }
  if (rc != 1) fail(c, "no plan");
  ++n_plans;
  if (p.bnd != (bnd ? 1 : 0) || p.inl != (inl ? 1 : 0)) fail(c, "bnd / inl flags");
  const Args a = {n3, nt, p.k_begin, p.k_end, p.kz, p.kspan, p.nchunk, p.nbw, p.bends, p.c0, p.nint};
  const int grid = p.nbw + p.nint;
  if (grid != nt * p.nchunk + (inl && !p.bends ? 2 * nt : 0)) fail(c, "(v) nbw + nint is not the grid");
  if (c.kz > 0 && !bnd && p.kz != c.kz) fail(c, "the forced kz was not taken");
  if (c.code == PFT_ZP_ENDS_FIRST && p.fallback) {
    Case ci = c;
    ci.code = PFT_ZP_INLINE;
    pft_zplan q;
    if (make(ci, &q) != 1) fail(c, "(iv) no PFT_K_INLINE plan");
    q.fallback = 1;
    if (memcmp(&p, &q, sizeof(p))) fail(c, "(iv) the fallback is not PFT_K_INLINE's plan");
  }
  if (c.code == PFT_ZP_ENDS_FIRST && !p.fallback && (!p.bends || p.nbw != 2 * nt || p.nchunk < 3))
    fail(c, "(iii) ends-first without its leading chunks");
  if (c.code == PFT_ZP_INLINE && (p.bends || p.nbw != 2 * nt || p.k_begin != 2 || p.k_end != n3 - 2))
    fail(c, "(ii) inline without its boundary chunks");
  if (!inl && p.nbw) fail(c, "leading workgroups without an inline boundary");

  if (nxt.size() < (size_t)nt * (n3 + 1)) nxt.resize((size_t)nt * (n3 + 1), 0);
  touched.clear();
  std::vector<int> lead((size_t)nt, 0);   // per tile: bit 0 the low end led, bit 1 the high end
  for (int b = 0; b < grid; ++b) {
    int tile, chunk, kb, ke;
    bool bw, bshort;
    pft_zplan_chunk(b, a.ntile, a.nchunk, a.nbw, a.bends, a.c0, a.nint, &tile, &chunk, &bw, &bshort);
    pft_zplan_planes(chunk, bshort, a.n3, a.k_begin, a.k_end, a.kz, a.kspan, &kb, &ke);
    ++n_wg;
    if (tile < 0 || tile >= nt) fail(c, "tile out of range", b);
    if (kb < 0 || ke > n3 || ke <= kb) fail(c, "(v) an empty chunk, or planes outside the slab", b);
    if (bw != (b < p.nbw)) fail(c, "leading workgroup flag", b);
    if (p.nbw == 0) {
      // the decode of a launch without leading workgroups (merson_stage) is the same
      int tile2, chunk2, kb2, ke2;
      pft_zplan_chunk_flat(b, a.ntile, a.nchunk, &tile2, &chunk2);
      pft_zplan_planes(chunk2, false, a.n3, a.k_begin, a.k_end, a.kz, a.kspan, &kb2, &ke2);
      if (tile2 != tile || kb2 != kb || ke2 != ke) fail(c, "the flat decode differs", b);
    }
    if (bw) {
      const int end = kb == 0 ? 1 : 2;
      if (p.bends) {
        // (iii)
        if (chunk != (end == 1 ? 0 : p.nchunk - 1) || ke - kb < 2 || (end == 2 && ke != n3)) fail(c, "(iii) a leading workgroup is no end chunk of two planes", b);
      } else if (!((kb == 0 && ke == 2) || (kb == n3 - 2 && ke == n3))) {
        fail(c, "(ii) a leading workgroup runs other planes than 0, 1 or n3-2, n3-1", b);
      }
      if (lead[tile] & end) fail(c, "an end of a tile led twice", b);
      lead[tile] |= end;
    } else if (inl && !p.bends && (kb < 2 || ke > n3 - 2)) {
      fail(c, "(ii) an interior workgroup outside [2, n3-2)", b);
    } else if (inl && p.bends && (chunk == 0 || chunk == p.nchunk - 1)) {
      fail(c, "(iii) an end chunk among the other workgroups", b);
    }
    int& e = nxt[(size_t)tile * (n3 + 1) + kb];
    if (e) fail(c, "(i) two workgroups start at one plane of a tile", b);
    e = ke;
    touched.push_back((size_t)tile * (n3 + 1) + kb);
  }
  // (i): per tile the chunks chain through each requested range, and there are no others
  long chained = 0;
  for (int t = 0; t < nt; ++t) {
    if (inl && lead[t] != 3) fail(c, "a tile's ends are not both led");
    if (overlap) {
      const int* e = &nxt[(size_t)t * (n3 + 1)];
      if (e[0] != 2 || e[1] != 3) fail(c, "the three-plane two-deep boundary launch changed");
      chained += 2;
      continue;
    }
    for (int r = 0; r < nr; ++r) {
      int k = r0[r];
      while (k < r1[r]) {
        const int e = nxt[(size_t)t * (n3 + 1) + k];
        if (e <= k || e > r1[r]) fail(c, "(i) a plane of the range is not run, or a chunk leaves the range");
        k = e;
        ++chained;
      }
    }
  }
  if (chained != grid) fail(c, "(i) workgroups outside the requested range");
  for (size_t i : touched) nxt[i] = 0;
}

// (vi) occ, ntile, nplanes, min_nch, ncu -> kz.  The first ten rows are the ones the cost model was
// moved with; the others were dumped from the loop it was moved from (pft_kernels.hip's chunk_kz
// before pft_zplan.h), compiled as it stood into a scratch program.
static const int KZ_TABLE[][6] = {
  {2, 80, 400, 1, 256, 67},
  {3, 80, 400, 1, 256, 45},
  {2, 320, 100, 1, 256, 34},
  {1, 50, 400, 1, 256, 80},
  {1, 50, 400, 3, 256, 80},
  {1, 220, 100, 1, 256, 100},
  {1, 220, 100, 3, 256, 34},
  {1, 5, 5, 3, 256, 1},
  {1, 5, 6, 3, 256, 2},
  {1, 5, 7, 3, 256, 1},
  {1, 1, 1, 1, 8, 1},
  {1, 1, 3, 3, 8, 1},
  {1, 1, 5, 3, 256, 1},
  {1, 1, 7, 1, 8, 1},
  {1, 1, 9, 3, 8, 3},
  {1, 1, 13, 1, 224, 1},
  {1, 1, 21, 3, 8, 3},
  {1, 1, 24, 3, 224, 2},
  {1, 1, 100, 1, 8, 13},
  {1, 1, 396, 3, 224, 2},
  {1, 3, 1, 1, 224, 1},
  {1, 3, 3, 3, 224, 1},
  {1, 3, 6, 1, 256, 1},
  {1, 3, 7, 1, 224, 1},
  {1, 3, 9, 3, 224, 3},
  {1, 3, 16, 1, 8, 8},
  {1, 3, 21, 3, 224, 3},
  {1, 3, 96, 1, 256, 2},
  {1, 3, 100, 1, 224, 2},
  {1, 3, 400, 1, 8, 80},
  {1, 7, 2, 3, 256, 1},
  {1, 7, 4, 1, 8, 4},
  {1, 7, 6, 3, 8, 2},
  {1, 7, 8, 3, 256, 2},
  {1, 7, 11, 3, 256, 3},
  {1, 7, 16, 1, 224, 1},
  {1, 7, 24, 1, 256, 1},
  {1, 7, 96, 3, 8, 32},
  {1, 7, 396, 1, 256, 11},
  {1, 7, 400, 1, 224, 13},
  {1, 8, 3, 1, 256, 1},
  {1, 8, 4, 1, 224, 1},
  {1, 8, 6, 3, 224, 2},
  {1, 8, 9, 1, 256, 1},
  {1, 8, 13, 1, 8, 13},
  {1, 8, 21, 1, 256, 1},
  {1, 8, 24, 3, 8, 8},
  {1, 8, 96, 3, 224, 4},
  {1, 8, 396, 3, 8, 132},
  {1, 9, 1, 1, 8, 1},
  {1, 9, 3, 3, 8, 1},
  {1, 9, 5, 3, 256, 1},
  {1, 9, 7, 1, 8, 7},
  {1, 9, 9, 3, 8, 3},
  {1, 9, 13, 1, 224, 1},
  {1, 9, 21, 3, 8, 7},
  {1, 9, 24, 3, 224, 2},
  {1, 9, 100, 1, 8, 25},
  {1, 9, 396, 3, 224, 18},
  {1, 50, 1, 1, 224, 1},
  {1, 50, 3, 3, 224, 1},
  {1, 50, 6, 1, 256, 2},
  {1, 50, 7, 1, 224, 2},
  {1, 50, 9, 3, 224, 3},
  {1, 50, 16, 1, 8, 16},
  {1, 50, 21, 3, 224, 6},
  {1, 50, 96, 1, 256, 20},
  {1, 50, 100, 1, 224, 25},
  {1, 50, 400, 1, 8, 200},
  {1, 80, 2, 3, 256, 1},
  {1, 80, 4, 1, 8, 4},
  {1, 80, 6, 3, 8, 2},
  {1, 80, 8, 3, 256, 3},
  {1, 80, 11, 3, 256, 4},
  {1, 80, 16, 1, 224, 8},
  {1, 80, 24, 1, 256, 8},
  {1, 80, 96, 3, 8, 32},
  {1, 80, 396, 1, 256, 132},
  {1, 80, 400, 1, 224, 29},
  {1, 220, 3, 1, 256, 3},
  {1, 220, 4, 1, 224, 4},
  {1, 220, 6, 3, 224, 2},
  {1, 220, 9, 1, 256, 9},
  {1, 220, 13, 1, 8, 13},
  {1, 220, 21, 1, 256, 21},
  {1, 220, 24, 3, 8, 8},
  {1, 220, 96, 3, 224, 32},
  {1, 220, 396, 3, 8, 132},
  {1, 320, 1, 1, 8, 1},
  {1, 320, 3, 3, 8, 1},
  {1, 320, 5, 3, 256, 1},
  {1, 320, 7, 1, 8, 7},
  {1, 320, 9, 3, 8, 3},
  {1, 320, 13, 1, 224, 7},
  {1, 320, 21, 3, 8, 7},
  {1, 320, 24, 3, 224, 8},
  {1, 320, 100, 1, 8, 100},
  {1, 320, 396, 3, 224, 99},
  {1, 800, 1, 1, 224, 1},
  {1, 800, 3, 3, 224, 1},
  {1, 800, 6, 1, 256, 6},
  {1, 800, 7, 1, 224, 7},
  {1, 800, 9, 3, 224, 3},
  {1, 800, 16, 1, 8, 16},
  {1, 800, 21, 3, 224, 7},
  {1, 800, 96, 1, 256, 48},
  {1, 800, 100, 1, 224, 100},
  {1, 800, 400, 1, 8, 400},
  {2, 1, 1, 3, 224, 1},
  {2, 1, 4, 1, 256, 1},
  {2, 1, 5, 1, 224, 1},
  {2, 1, 7, 3, 224, 1},
  {2, 1, 11, 1, 8, 1},
  {2, 1, 13, 3, 224, 5},
  {2, 1, 21, 3, 256, 3},
  {2, 1, 100, 3, 8, 7},
  {2, 1, 400, 3, 8, 25},
  {2, 3, 1, 3, 224, 1},
  {2, 3, 4, 1, 256, 1},
  {2, 3, 5, 1, 224, 1},
  {2, 3, 7, 3, 224, 1},
  {2, 3, 11, 1, 8, 3},
  {2, 3, 13, 3, 224, 5},
  {2, 3, 21, 3, 256, 3},
  {2, 3, 100, 3, 8, 20},
  {2, 3, 400, 3, 8, 80},
  {2, 7, 1, 3, 224, 1},
  {2, 7, 4, 1, 256, 1},
  {2, 7, 5, 1, 224, 1},
  {2, 7, 7, 3, 224, 1},
  {2, 7, 11, 1, 8, 6},
  {2, 7, 13, 3, 224, 5},
  {2, 7, 21, 3, 256, 3},
  {2, 7, 100, 3, 8, 25},
  {2, 7, 400, 3, 8, 45},
  {2, 8, 1, 3, 224, 1},
  {2, 8, 4, 1, 256, 1},
  {2, 8, 5, 1, 224, 1},
  {2, 8, 7, 3, 224, 1},
  {2, 8, 11, 1, 8, 6},
  {2, 8, 13, 3, 224, 5},
  {2, 8, 21, 3, 256, 3},
  {2, 8, 100, 3, 8, 25},
  {2, 8, 400, 3, 8, 100},
  {2, 9, 1, 3, 224, 1},
  {2, 9, 4, 1, 256, 1},
  {2, 9, 5, 1, 224, 1},
  {2, 9, 7, 3, 224, 1},
  {2, 9, 11, 1, 8, 4},
  {2, 9, 13, 3, 224, 5},
  {2, 9, 21, 3, 256, 3},
  {2, 9, 100, 3, 8, 20},
  {2, 9, 400, 3, 8, 80},
  {2, 50, 1, 3, 224, 1},
  {2, 50, 4, 1, 256, 1},
  {2, 50, 5, 1, 224, 1},
  {2, 50, 7, 3, 224, 1},
  {2, 50, 11, 1, 8, 11},
  {2, 50, 13, 3, 224, 5},
  {2, 50, 21, 3, 256, 3},
  {2, 50, 100, 3, 8, 34},
  {2, 50, 400, 3, 8, 134},
  {2, 80, 1, 3, 224, 1},
  {2, 80, 4, 1, 256, 1},
  {2, 80, 5, 1, 224, 1},
  {2, 80, 7, 3, 224, 1},
  {2, 80, 11, 1, 8, 11},
  {2, 80, 13, 3, 224, 5},
  {2, 80, 21, 3, 256, 6},
  {2, 80, 100, 3, 8, 34},
  {2, 80, 400, 3, 8, 134},
  {2, 220, 1, 3, 224, 1},
  {2, 220, 4, 1, 256, 2},
  {2, 220, 5, 1, 224, 3},
  {2, 220, 7, 3, 224, 1},
  {2, 220, 11, 1, 8, 11},
  {2, 220, 13, 3, 224, 5},
  {2, 220, 21, 3, 256, 6},
  {2, 220, 100, 3, 8, 34},
  {2, 220, 400, 3, 8, 134},
  {2, 320, 1, 3, 224, 1},
  {2, 320, 4, 1, 256, 4},
  {2, 320, 5, 1, 224, 5},
  {2, 320, 7, 3, 224, 1},
  {2, 320, 11, 1, 8, 11},
  {2, 320, 13, 3, 224, 5},
  {2, 320, 21, 3, 256, 7},
  {2, 320, 100, 3, 8, 34},
  {2, 320, 400, 3, 8, 134},
  {2, 800, 1, 3, 224, 1},
  {2, 800, 4, 1, 256, 4},
  {2, 800, 5, 1, 224, 5},
  {2, 800, 7, 3, 224, 1},
  {2, 800, 11, 1, 8, 11},
  {2, 800, 13, 3, 224, 5},
  {2, 800, 21, 3, 256, 7},
  {2, 800, 100, 3, 8, 34},
  {2, 800, 400, 3, 8, 134},
  {3, 1, 2, 3, 8, 1},
  {3, 1, 4, 3, 256, 1},
  {3, 1, 6, 1, 8, 1},
  {3, 1, 8, 3, 8, 2},
  {3, 1, 11, 1, 256, 1},
  {3, 1, 16, 3, 256, 2},
  {3, 1, 24, 1, 224, 1},
  {3, 1, 396, 1, 8, 18},
  {3, 3, 2, 1, 256, 1},
  {3, 3, 3, 1, 224, 1},
  {3, 3, 5, 3, 224, 1},
  {3, 3, 8, 1, 256, 1},
  {3, 3, 9, 1, 224, 1},
  {3, 3, 13, 3, 256, 5},
  {3, 3, 24, 1, 8, 3},
  {3, 3, 100, 3, 256, 2},
  {3, 7, 1, 3, 256, 1},
  {3, 7, 3, 1, 8, 1},
  {3, 7, 5, 3, 8, 1},
  {3, 7, 7, 3, 256, 1},
  {3, 7, 9, 1, 8, 3},
  {3, 7, 11, 3, 224, 3},
  {3, 7, 21, 1, 224, 1},
  {3, 7, 96, 1, 224, 1},
  {3, 7, 400, 3, 256, 4},
  {3, 8, 2, 3, 224, 1},
  {3, 8, 5, 1, 256, 1},
  {3, 8, 6, 1, 224, 1},
  {3, 8, 8, 3, 224, 2},
  {3, 8, 11, 3, 8, 4},
  {3, 8, 21, 1, 8, 7},
  {3, 8, 96, 1, 8, 32},
  {3, 8, 396, 1, 224, 5},
  {3, 9, 2, 3, 8, 1},
  {3, 9, 4, 3, 256, 1},
  {3, 9, 6, 1, 8, 3},
  {3, 9, 8, 3, 8, 3},
  {3, 9, 11, 1, 256, 1},
  {3, 9, 16, 3, 256, 2},
  {3, 9, 24, 1, 224, 1},
  {3, 9, 396, 1, 8, 66},
  {3, 50, 2, 1, 256, 1},
  {3, 50, 3, 1, 224, 1},
  {3, 50, 5, 3, 224, 1},
  {3, 50, 8, 1, 256, 1},
  {3, 50, 9, 1, 224, 1},
  {3, 50, 13, 3, 256, 5},
  {3, 50, 24, 1, 8, 24},
  {3, 50, 100, 3, 256, 7},
  {3, 80, 1, 3, 256, 1},
  {3, 80, 3, 1, 8, 3},
  {3, 80, 5, 3, 8, 1},
  {3, 80, 7, 3, 256, 1},
  {3, 80, 9, 1, 8, 9},
  {3, 80, 11, 3, 224, 3},
  {3, 80, 21, 1, 224, 3},
  {3, 80, 96, 1, 224, 12},
  {3, 80, 400, 3, 256, 45},
  {3, 220, 2, 3, 224, 1},
  {3, 220, 5, 1, 256, 2},
  {3, 220, 6, 1, 224, 2},
  {3, 220, 8, 3, 224, 3},
  {3, 220, 11, 3, 8, 4},
  {3, 220, 21, 1, 8, 21},
  {3, 220, 96, 1, 8, 96},
  {3, 220, 396, 1, 224, 132},
  {3, 320, 2, 3, 8, 1},
  {3, 320, 4, 3, 256, 1},
  {3, 320, 6, 1, 8, 6},
  {3, 320, 8, 3, 8, 3},
  {3, 320, 11, 1, 256, 6},
  {3, 320, 16, 3, 256, 4},
  {3, 320, 24, 1, 224, 12},
  {3, 320, 396, 1, 8, 396},
  {3, 800, 2, 1, 256, 2},
  {3, 800, 3, 1, 224, 3},
  {3, 800, 5, 3, 224, 1},
  {3, 800, 8, 1, 256, 8},
  {3, 800, 9, 1, 224, 9},
  {3, 800, 13, 3, 256, 5},
  {3, 800, 24, 1, 8, 24},
  {3, 800, 100, 3, 256, 34},
  {4, 1, 1, 1, 8, 1},
  {4, 1, 3, 3, 8, 1},
  {4, 1, 5, 3, 256, 1},
  {4, 1, 7, 1, 8, 1},
  {4, 1, 9, 3, 8, 3},
  {4, 1, 13, 1, 224, 1},
  {4, 1, 21, 3, 8, 3},
  {4, 1, 24, 3, 224, 2},
  {4, 1, 100, 1, 8, 4},
  {4, 1, 396, 3, 224, 2},
  {4, 3, 1, 1, 224, 1},
  {4, 3, 3, 3, 224, 1},
  {4, 3, 6, 1, 256, 1},
  {4, 3, 7, 1, 224, 1},
  {4, 3, 9, 3, 224, 3},
  {4, 3, 16, 1, 8, 2},
  {4, 3, 21, 3, 224, 3},
  {4, 3, 96, 1, 256, 1},
  {4, 3, 100, 1, 224, 1},
  {4, 3, 400, 1, 8, 40},
  {4, 7, 2, 3, 256, 1},
  {4, 7, 4, 1, 8, 1},
  {4, 7, 6, 3, 8, 2},
  {4, 7, 8, 3, 256, 2},
  {4, 7, 11, 3, 256, 3},
  {4, 7, 16, 1, 224, 1},
  {4, 7, 24, 1, 256, 1},
  {4, 7, 96, 3, 8, 12},
  {4, 7, 396, 1, 256, 3},
  {4, 7, 400, 1, 224, 4},
  {4, 8, 3, 1, 256, 1},
  {4, 8, 4, 1, 224, 1},
  {4, 8, 6, 3, 224, 2},
  {4, 8, 9, 1, 256, 1},
  {4, 8, 13, 1, 8, 4},
  {4, 8, 21, 1, 256, 1},
  {4, 8, 24, 3, 8, 6},
  {4, 8, 96, 3, 224, 2},
  {4, 8, 396, 3, 8, 99},
  {4, 9, 1, 1, 8, 1},
  {4, 9, 3, 3, 8, 1},
  {4, 9, 5, 3, 256, 1},
  {4, 9, 7, 1, 8, 3},
  {4, 9, 9, 3, 8, 3},
  {4, 9, 13, 1, 224, 1},
  {4, 9, 21, 3, 8, 7},
  {4, 9, 24, 3, 224, 2},
  {4, 9, 100, 1, 8, 25},
  {4, 9, 396, 3, 224, 4},
  {4, 50, 1, 1, 224, 1},
  {4, 50, 3, 3, 224, 1},
  {4, 50, 6, 1, 256, 1},
  {4, 50, 7, 1, 224, 1},
  {4, 50, 9, 3, 224, 3},
  {4, 50, 16, 1, 8, 16},
  {4, 50, 21, 3, 224, 3},
  {4, 50, 96, 1, 256, 5},
  {4, 50, 100, 1, 224, 6},
  {4, 50, 400, 1, 8, 200},
  {4, 80, 2, 3, 256, 1},
  {4, 80, 4, 1, 8, 4},
  {4, 80, 6, 3, 8, 2},
  {4, 80, 8, 3, 256, 2},
  {4, 80, 11, 3, 256, 3},
  {4, 80, 16, 1, 224, 2},
  {4, 80, 24, 1, 256, 2},
  {4, 80, 96, 3, 8, 32},
  {4, 80, 396, 1, 256, 33},
  {4, 80, 400, 1, 224, 37},
  {4, 220, 3, 1, 256, 1},
  {4, 220, 4, 1, 224, 1},
  {4, 220, 6, 3, 224, 2},
  {4, 220, 9, 1, 256, 3},
  {4, 220, 13, 1, 8, 13},
  {4, 220, 21, 1, 256, 6},
  {4, 220, 24, 3, 8, 8},
  {4, 220, 96, 3, 224, 24},
  {4, 220, 396, 3, 8, 132},
  {4, 320, 1, 1, 8, 1},
  {4, 320, 3, 3, 8, 1},
  {4, 320, 5, 3, 256, 1},
  {4, 320, 7, 1, 8, 7},
  {4, 320, 9, 3, 8, 3},
  {4, 320, 13, 1, 224, 7},
  {4, 320, 21, 3, 8, 7},
  {4, 320, 24, 3, 224, 8},
  {4, 320, 100, 1, 8, 100},
  {4, 320, 396, 3, 224, 99},
  {4, 800, 1, 1, 224, 1},
  {4, 800, 3, 3, 224, 1},
  {4, 800, 6, 1, 256, 6},
  {4, 800, 7, 1, 224, 7},
  {4, 800, 9, 3, 224, 3},
  {4, 800, 16, 1, 8, 16},
  {4, 800, 21, 3, 224, 7},
  {4, 800, 96, 1, 256, 48},
  {4, 800, 100, 1, 224, 100},
  {4, 800, 400, 1, 8, 400},
};

int main()
{
  for (const auto& r : KZ_TABLE) {
    const int kz = pft_zplan_kz(r[0], r[1], r[2], r[3], r[4]);
    if (kz != r[5]) {
      fprintf(stderr, "zplan_check: (vi) pft_zplan_kz(%d, %d, %d, %d, %d) = %d, expected %d\n", r[0], r[1], r[2], r[3], r[4], kz, r[5]);
      return 1;
    }
  }
  // xcd_remap is a bijection of [0, n)
  for (int n = 1; n <= 70; ++n) {
    std::vector<int> seen((size_t)n, 0);
    for (int b = 0; b < n; ++b) {
      const int l = xcd_remap(b, n);
      if (l < 0 || l >= n || seen[l]++) {
        fprintf(stderr, "zplan_check: xcd_remap(%d, %d) = %d\n", b, n, l);
        return 1;
      }
    }
  }
  std::vector<int> n3s;
  for (int n3 = 1; n3 <= 24; ++n3) n3s.push_back(n3);
  n3s.push_back(100);
  n3s.push_back(400);
  const int ntiles[] = {1, 3, 7, 8, 9, 50, 220};
  const int ncus[] = {8, 256};
  for (int n3 : n3s) {
    // every range code, and explicit ranges: the interiors of the two splits, a range clamped at
    // the top, one plane, two empty ones
    const int ranges[][2] = {{-1, -1}, {PFT_ZP_BOUNDARY, 0}, {PFT_ZP_BOUNDARY2, 0}, {PFT_ZP_INLINE, 0}, {PFT_ZP_ENDS_FIRST, 0},
                             {1, n3 - 1}, {2, n3 - 2}, {0, n3 + 3}, {n3 / 2, n3 / 2 + 1}, {3, 3}, {n3, 2}};
    for (int nt : ntiles)
      for (int occ = 1; occ <= 3; ++occ)
        for (int ncu : ncus)
          for (int kz = 0; kz <= n3 + 1; ++kz) {
            // a forced kz leaves the cost model, and with it occ and ncu, out of the plan
            // (pft_zplan_make reads them through pft_zplan_auto_kz alone): those are enumerated
            // with the automatic kz only
            if (kz > 0 && (occ != 1 || ncu != 8)) continue;
            for (const auto& r : ranges)
              for (int depths = 2; depths <= 3; ++depths) {   // pair launches (depth 2), stage launches (1 and 2)
                if (depths == 2 && r[0] >= 0) continue;       // (explicit ranges do not look at it)
                const Case c = {r[0], r[1], n3, nt, kz, occ, ncu, depths};
                check(c);
              }
          }
  }
  printf("%ld %ld\n", n_plans, n_wg);
  return 0;
}
