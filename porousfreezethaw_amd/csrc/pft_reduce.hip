// pft_reduce.hip -- reductions over the resident state: the ice diagnostics (diag_kernel, f5) and
// the exact means and z-profiles (means_kernel, f6), the formula diagnostics (formula_kernel, f12)
// the histograms of formula values (hist_kernel, f13) and the 2-D maps of formula values (map_kernel,
// f15), with their host API.
#include "pft_slab.h"

#include "../../include/pft_formula.h"
#include "../../include/pft_hist.h"
#include "../../include/pft_map.h"
#define PFT_IC_NO_CP   // no loop with a cell's value as its trip count is compiled into formula_kernel
#include "pft_ic_ops.h"

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------
// f5: the ice diagnostics of a state (pft_diag.h) -- a streaming reduction over the interior of
// the three fields, each one contiguous run of n = n3 * plane doubles from plane 1 (no x/y ghosts).
//
// Everything is an integer: counts are added as 64-bit integers, maxima and minima go through
// diag_key, a 64-bit key that orders every non-NaN double as the double orders (and -0.0 below
// +0.0), so the same bits come out for any grid, chunking or arrival order.  Key 0 belongs to no
// non-NaN double: a zeroed accumulator means "no value yet", and the minimum is kept as the maximum
// of the complemented key, so one hipMemsetAsync per call resets every word.
//
// Work: the run is cut into 16-byte pairs (pair q = elements 2q - head, 2q - head + 1; head = 1
// if the run started on an odd multiple of 8 bytes -- with the slab's layout it does not -- and the
// first and the last pair may hold one element).  Workgroup b takes per_wg consecutive pairs and
// indexes its elements from its first pair's (32-bit r); per iteration each wave takes 512
// consecutive elements, four 16-byte loads per lane and field, all issued before the first use, so
// a wave meets the planes in ascending order.  Where the 512 lie inside the run (all but the first
// and last iteration of the grid) no element is tested for validity; elsewhere each is loaded alone
// under its own test.  Counts come from __ballot and popcount and stay in scalar registers; the ice
// count of the iteration goes to its plane -- one add when the 512 elements lie in one plane, else
// one ballot round per plane touched -- into an LDS window of the workgroup's first PFT_DIAG_WIN
// planes (past the window: the plane's global word).  At the end the keys are reduced across the
// lanes and, through LDS, across the four waves: one set of global atomics per workgroup, plus
// one per plane it touched.  (A first version with one pair per lane and iteration and 64-bit
// bookkeeping ran at 3.5 TB/s, bound by scalar instruction issue: DESIGN.md section 7, f5.)
#define PFT_DBLOCK 256
#define PFT_DIAG_UNROLL 4                               // 16-byte loads per lane, field and iteration
#define PFT_DIAG_WAVE_ELEMS (128 * PFT_DIAG_UNROLL)    // elements of a wave's iteration
#define PFT_DIAG_WG_PAIRS (PFT_DBLOCK * PFT_DIAG_UNROLL)
#define PFT_DIAG_HEAD 16   // accumulator words before the per-plane counts
#define PFT_DIAG_WIN 64
enum { DG_ICE = 0, DG_PORE, DG_ICE_PORE, DG_NONFINITE, DG_ICE_U, DG_U_MAX, DG_U_MIN, DG_P_MAX, DG_P_MIN, DG_WORDS };

__host__ __device__ static inline unsigned long long diag_key(double x)
{
  unsigned long long b;
  memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | (1ULL << 63));
}
static double diag_unkey(unsigned long long k)
{
  const unsigned long long b = (k >> 63) ? (k & ~(1ULL << 63)) : ~k;
  double x;
  memcpy(&x, &b, 8);
  return x;
}

__device__ __forceinline__ bool diag_finite(double x) { return fabs(x) < __builtin_inf(); }   // false on NaN

struct DiagState {
  unsigned long long c_ice, c_pore, c_both, c_nf;     // wave-uniform counts
  unsigned long long iu, umax, umin, pmax, pmin;      // per-lane keys
  int k, lo, hi;   // the wave's running plane: index from the workgroup's first, elements [lo, hi) (r)
};

// one iteration of a wave: elements r0 .. r0 + 511 of the workgroup (of them [r_lo, r_hi) exist;
// FULL: all do).  fu/fp/fg point at the workgroup's element 0.
template <bool FULL>
__device__ __forceinline__ void diag_iter(DiagState& st, const double* __restrict__ fu, const double* __restrict__ fp,
                                          const double* __restrict__ fg, int r0, int r_lo, int r_hi, int plane,
                                          int lane, double p_thr, double gl_thr, unsigned long long* s_win,
                                          unsigned long long* __restrict__ acc_planes)
{
  constexpr int NE = 2 * PFT_DIAG_UNROLL;
  double u[NE], p[NE], g[NE];
  bool v[NE], ice[NE];
#pragma unroll
  for (int j = 0; j < PFT_DIAG_UNROLL; ++j) {
    const int r = r0 + 128 * j + 2 * lane;
    if (FULL) {
      const double2 a = *reinterpret_cast<const double2*>(fu + r);
      const double2 b = *reinterpret_cast<const double2*>(fp + r);
      const double2 c = *reinterpret_cast<const double2*>(fg + r);
      u[2 * j] = a.x, u[2 * j + 1] = a.y, p[2 * j] = b.x, p[2 * j + 1] = b.y, g[2 * j] = c.x, g[2 * j + 1] = c.y;
      v[2 * j] = v[2 * j + 1] = true;
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool ok = r + i >= r_lo && r + i < r_hi;
        v[2 * j + i] = ok;
        u[2 * j + i] = ok ? fu[r + i] : 0.0;
        p[2 * j + i] = ok ? fp[r + i] : 0.0;
        g[2 * j + i] = ok ? fg[r + i] : 0.0;
      }
    }
  }
  unsigned it_ice = 0;
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    // ordered comparisons: false on NaN
    ice[i] = v[i] && p[i] > p_thr;
    const bool por = v[i] && g[i] < gl_thr;
    const bool nf = v[i] && !(diag_finite(u[i]) && diag_finite(p[i]) && diag_finite(g[i]));
    it_ice += (unsigned)__popcll(__ballot(ice[i]));
    st.c_pore += __popcll(__ballot(por));
    st.c_both += __popcll(__ballot(ice[i] && por));
    st.c_nf += __popcll(__ballot(nf));
    if (v[i] && u[i] == u[i]) {
      const unsigned long long k = diag_key(u[i]);
      st.umax = k > st.umax ? k : st.umax;
      st.umin = ~k > st.umin ? ~k : st.umin;
      if (ice[i]) {
        const unsigned long long a = (unsigned long long)__double_as_longlong(fabs(u[i]));
        st.iu = a > st.iu ? a : st.iu;   // non-negative doubles order as their bits
      }
    }
    if (v[i] && p[i] == p[i]) {
      const unsigned long long k = diag_key(p[i]);
      st.pmax = k > st.pmax ? k : st.pmax;
      st.pmin = ~k > st.pmin ? ~k : st.pmin;
    }
  }
  st.c_ice += it_ice;
  // the ice counts of the planes the wave's existing elements [w0, w1] lie in
  const int w0 = FULL ? r0 : (r0 > r_lo ? r0 : r_lo);
  const int w1 = (FULL ? r0 + PFT_DIAG_WAVE_ELEMS : (r0 + PFT_DIAG_WAVE_ELEMS < r_hi ? r0 + PFT_DIAG_WAVE_ELEMS : r_hi)) - 1;
  if (w1 < w0) return;
  while (w0 >= st.hi) {
    ++st.k;
    st.lo = st.hi;
    st.hi += plane;
  }
  const bool one_plane = w1 < st.hi;
  while (true) {
    unsigned c = it_ice;
    if (!one_plane) {
      c = 0;
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const int r = r0 + 128 * (i >> 1) + 2 * lane + (i & 1);
        c += (unsigned)__popcll(__ballot(ice[i] && r >= st.lo && r < st.hi));
      }
    }
    if (lane == 0 && c) {
      if (st.k < PFT_DIAG_WIN)
        atomicAdd(&s_win[st.k], (unsigned long long)c);
      else
        atomicAdd(&acc_planes[st.k], (unsigned long long)c);
    }
    if (w1 < st.hi) break;
    ++st.k;
    st.lo = st.hi;
    st.hi += plane;
  }
}

__global__ __launch_bounds__(PFT_DBLOCK) void diag_kernel(const double* __restrict__ fu, const double* __restrict__ fp,
                                                          const double* __restrict__ fg, long n, int plane, int head,
                                                          long nq, long per_wg, double p_thr, double gl_thr,
                                                          unsigned long long* __restrict__ acc)
{
  __shared__ unsigned long long s_win[PFT_DIAG_WIN];
  __shared__ unsigned long long s_red[PFT_DBLOCK / 64][DG_WORDS];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long q_begin = (long)blockIdx.x * per_wg;
  const long q_end = q_begin + per_wg < nq ? q_begin + per_wg : nq;
  for (int i = threadIdx.x; i < PFT_DIAG_WIN; i += PFT_DBLOCK) s_win[i] = 0;
  __syncthreads();
  // the workgroup's elements r = 0 .. span - 1 stand for e_base + r of the run; of them [r_lo, r_hi)
  // exist (e_base = -1: the slot before the run; the last pair's second slot may lie past its end)
  const long e_base = 2 * q_begin - head;
  const int span = (int)(2 * (q_end - q_begin));
  const int r_lo = e_base < 0 ? 1 : 0;
  const int r_hi = n - e_base < span ? (int)(n - e_base) : span;
  const long k_base = (e_base > 0 ? e_base : 0) / plane;   // the first plane this workgroup touches
  DiagState st;
  st.c_ice = st.c_pore = st.c_both = st.c_nf = 0;
  st.iu = st.umax = st.umin = st.pmax = st.pmin = 0;
  st.k = 0;
  st.lo = (int)(k_base * plane - e_base);
  st.hi = st.lo + plane;
  const double* wu = fu + e_base;   // (e_base = -1: one before the run, never read at r = 0)
  const double* wp = fp + e_base;
  const double* wg = fg + e_base;
  unsigned long long* acc_planes = acc + PFT_DIAG_HEAD + k_base;

  for (int r0 = PFT_DIAG_WAVE_ELEMS * wave; r0 < span; r0 += PFT_DIAG_WAVE_ELEMS * (PFT_DBLOCK / 64)) {
    if (r0 >= r_lo && r0 + PFT_DIAG_WAVE_ELEMS <= r_hi)
      diag_iter<true>(st, wu, wp, wg, r0, r_lo, r_hi, plane, lane, p_thr, gl_thr, s_win, acc_planes);
    else
      diag_iter<false>(st, wu, wp, wg, r0, r_lo, r_hi, plane, lane, p_thr, gl_thr, s_win, acc_planes);
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long o;
    o = __shfl_xor(st.iu, off, 64), st.iu = o > st.iu ? o : st.iu;
    o = __shfl_xor(st.umax, off, 64), st.umax = o > st.umax ? o : st.umax;
    o = __shfl_xor(st.umin, off, 64), st.umin = o > st.umin ? o : st.umin;
    o = __shfl_xor(st.pmax, off, 64), st.pmax = o > st.pmax ? o : st.pmax;
    o = __shfl_xor(st.pmin, off, 64), st.pmin = o > st.pmin ? o : st.pmin;
  }
  if (lane == 0) {
    unsigned long long* r = s_red[wave];
    r[DG_ICE] = st.c_ice, r[DG_PORE] = st.c_pore, r[DG_ICE_PORE] = st.c_both, r[DG_NONFINITE] = st.c_nf;
    r[DG_ICE_U] = st.iu, r[DG_U_MAX] = st.umax, r[DG_U_MIN] = st.umin, r[DG_P_MAX] = st.pmax, r[DG_P_MIN] = st.pmin;
  }
  __syncthreads();
  if (threadIdx.x < DG_WORDS) {
    // one thread per accumulator word: the waves' partials, then one atomic
    const int w = threadIdx.x;
    unsigned long long x = s_red[0][w];
    for (int i = 1; i < PFT_DBLOCK / 64; ++i) {
      const unsigned long long o = s_red[i][w];
      x = w <= DG_NONFINITE ? x + o : (o > x ? o : x);
    }
    if (x) {
      if (w <= DG_NONFINITE)
        atomicAdd(&acc[w], x);
      else
        atomicMax(&acc[w], x);
    }
  }
  if (threadIdx.x >= 64 && threadIdx.x < 64 + PFT_DIAG_WIN) {
    const int t = threadIdx.x - 64;
    const unsigned long long x = s_win[t];
    if (x) atomicAdd(&acc_planes[t], x);
  }
}

// interior planes 1..n3 of u in buffer buf, one contiguous run (p and gl follow at s->fs and 2 s->fs;
// the ghost planes 0, n3+1 and the far planes are never read); *head = 1 when the run starts on an
// odd multiple of 8 bytes (the field stride is even: the same for u, p, gl)
static const double* slab_fields(const pft_slab* s, int buf, int* head)
{
  const double* fu = s->buf[buf] + s->plane;
  *head = (int)(((uintptr_t)fu >> 3) & 1);
  return fu;
}

// The cut of the slab's planes into work items (f6, f12, f13): at most `cap` workgroups (8 per CU),
// each inside one plane: a plane is cut into as many segments as the cap allows, each a whole number
// of workgroup iterations; with fewer workgroups than planes a workgroup takes several planes in
// turn.  An item is segment j of plane k, item = k * segs + j.
static void plane_work_cut(const pft_slab* s, int* segs, int* seg_len, unsigned* wgs)
{
  const long plane = s->plane, n3 = s->d.n3;
  const long cap = s->diag_wgs > 0 ? s->diag_wgs : 8L * (s->n_cu > 0 ? s->n_cu : 256);
  const long wg_elems = 2L * PFT_DIAG_WG_PAIRS;
  long want = cap / n3;
  if (want < 1) want = 1;
  const long len = ((plane + want - 1) / want + wg_elems - 1) / wg_elems * wg_elems;
  const long items = (plane + len - 1) / len * n3;
  *segs = (int)((plane + len - 1) / len);
  *seg_len = (int)len;
  *wgs = (unsigned)(items < cap ? items : cap);
}

extern "C" {

int pft_slab_diag(pft_slab* s, int buf, const pft_diag_opts* opts, pft_diag* out, long long* ice_per_plane)
{
  if (!s || !out || buf < 0 || buf >= PFT_BUF_COUNT) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_diag");
  const long plane = s->plane, n = (long)s->d.n3 * plane;
  const size_t bytes = sizeof(unsigned long long) * (size_t)(PFT_DIAG_HEAD + s->d.n3);
  if (!s->diag_dev) HIPCHK(hipMalloc((void**)&s->diag_dev, bytes));
  if (!s->diag_host) HIPCHK(hipHostMalloc((void**)&s->diag_host, bytes, hipHostMallocDefault));
  int head;
  const double* fu = slab_fields(s, buf, &head);
  const long nq = (n + head + 1) / 2;
  if (plane > (1L << 30)) return -2;   // (the kernel's 32-bit plane bounds)
  // at most `cap` workgroups (all resident at once: 8 per CU), each a whole number of iterations
  const long cap = s->diag_wgs > 0 ? s->diag_wgs : 8L * (s->n_cu > 0 ? s->n_cu : 256);
  long wgs = (nq + PFT_DIAG_WG_PAIRS - 1) / PFT_DIAG_WG_PAIRS;
  if (wgs > cap) wgs = cap;
  const long wgs_min = (nq >> 29) + 1;   // a workgroup indexes its elements with 32 bits
  if (wgs < wgs_min) wgs = wgs_min;
  const long per_wg = ((nq + wgs - 1) / wgs + PFT_DIAG_WG_PAIRS - 1) / PFT_DIAG_WG_PAIRS * PFT_DIAG_WG_PAIRS;
  wgs = (nq + per_wg - 1) / per_wg;
  const double p_thr = opts ? opts->p_thr : 0.5, gl_thr = opts ? opts->gl_thr : 0.5;
  // no state carries over between calls: every accumulator word is zeroed on the stream first
  HIPCHK(hipMemsetAsync(s->diag_dev, 0, bytes, s->stream));
  if (s->diag_timing) HIPCHK(hipEventRecord(s->ev_diag[0], s->stream));
  diag_kernel<<<(unsigned)wgs, PFT_DBLOCK, 0, s->stream>>>(fu, fu + s->fs, fu + 2 * s->fs, n, (int)plane, head, nq, per_wg,
                                                           p_thr, gl_thr, s->diag_dev);
  HIPCHK(hipGetLastError());
  if (s->diag_timing) HIPCHK(hipEventRecord(s->ev_diag[1], s->stream));
  HIPCHK(hipMemcpyAsync(s->diag_host, s->diag_dev, bytes, hipMemcpyDeviceToHost, s->stream));
  // the slab's bounded wait: an ipc peer's timeout or an aborted communicator ends it, as for the
  // error norm
  const int rc = slab_wait(s, nullptr, "pft_slab_diag");
  if (rc) return rc;
  const unsigned long long* h = s->diag_host;
  out->cells = n;
  out->ice = (long long)h[DG_ICE];
  out->pore = (long long)h[DG_PORE];
  out->ice_pore = (long long)h[DG_ICE_PORE];
  out->nonfinite = (long long)h[DG_NONFINITE];
  memcpy(&out->ice_u_maxabs, &h[DG_ICE_U], 8);
  const double inf = __builtin_inf();
  out->u_max = h[DG_U_MAX] ? diag_unkey(h[DG_U_MAX]) : -inf;
  out->u_min = h[DG_U_MIN] ? diag_unkey(~h[DG_U_MIN]) : inf;
  out->p_max = h[DG_P_MAX] ? diag_unkey(h[DG_P_MAX]) : -inf;
  out->p_min = h[DG_P_MIN] ? diag_unkey(~h[DG_P_MIN]) : inf;
  if (ice_per_plane)
    for (int k = 0; k < s->d.n3; ++k) ice_per_plane[k] = (long long)h[PFT_DIAG_HEAD + k];
  return 0;
}

int pft_slab_diag_timing(pft_slab* s, int on) { return slab_timing_set(s, &pft_slab::diag_timing, &pft_slab::ev_diag, on); }

int pft_slab_diag_last_ms(pft_slab* s, double* ms) { return slab_timing_ms(s, &pft_slab::diag_timing, &pft_slab::ev_diag, ms); }

}  // extern "C"

// ------------------------------------------------------------------------------------------
// f6: the exact sums of a state (pft_means.h) -- the same streaming read as diag_kernel, but every
// double is split into its three 32-bit digits (pft_means.h: word index c, digits of M << s) and
// the digits are added as 64-bit integers, so the words that come out are those of pft_means_host
// for any grid, chunking or arrival order.  No floating-point add, no compare-and-swap.
//
// Work: an item is a contiguous segment (seg_len elements, a multiple of a workgroup's iteration)
// of one interior plane; a workgroup takes items blockIdx.x, + gridDim.x, ... and for each one
// accumulates into an LDS copy of a pft_means record (268 words, 2 144 bytes), then adds its
// non-zero words to that plane's record in global memory: one integer atomic per word, the
// workgroups of different planes on different words.  means_total_kernel adds the planes' records.
// An item is read as diag_kernel reads its share: 16-byte pairs, per iteration each wave 512
// consecutive elements, four 16-byte loads per lane and field all issued before the first use;
// where the 512 do not all lie inside the item (its first and last iteration at most) each element
// is loaded alone under its own test.
//
// Contention is taken out on chip.  u -- and p away from the interface's tails -- lies in one
// 32-exponent window for every lane (word 32 for anything in [4, 2^34)), so a wave keeps a
// wave-uniform current word index `cur` per summand (MeansPair: the sum over all cells and the
// masked sum share the summand's digits) and each lane adds its digits to three 64-bit registers
// per sum.  Inactive lanes (zeros, NaN, +-Inf, slots outside the item) have zero digits and do not
// disturb that.  One ballot per iteration and summand tells whether some active lane has another
// index; only then the eight slots are taken one by one: a slot none of whose active lanes is at
// `cur` flushes the registers (a shuffle reduction, then lane 0 adds to LDS) and moves `cur` to
// its first active lane's index; lanes at `cur` add in registers, the others add their digits to
// LDS with per-lane 64-bit atomics.  Both ways add the same integers to the same words.  A second
// ballot asks whether any active value is negative: without one (u in kelvin, p in [0, 1]) the
// 32-bit digits are added as they are, with no negation and 32-bit selects for the masked sum.
// A lane adds at most plane / 256 + 8 <= 2^22 + 8 digits below 2^32 between two flushes (an item
// is at most a plane, PFT_MEANS_MAX_PLANE, and ends with a flush), so the wave's sum of 64 lanes
// stays below 2^61; an LDS word takes a workgroup's share of one plane and a global word at most
// 2^31 - 1 cells' digits: below 2^63.
#define PFT_MEANS_REC (PFT_MEAN_COUNT * (PFT_XSUM_WORDS + 1))   // 64-bit words of a pft_means: n[4], sum[4][66]
#define PFT_MEANS_MAX_PLANE (1L << 30)
static_assert(sizeof(pft_means) == 8 * PFT_MEANS_REC, "pft_means is n[4] then sum[4][66], no padding");

struct MeansPair {
  long long a0, a1, a2;   // per lane: the digits added for the sum over all cells, words cur .. cur + 2
  long long m0, m1, m2;   // the same for the masked sum
  int cur;                // wave-uniform, 0 .. 63; kept across flushes (the first guess: the word of
                          // u near 273 and of p near 1, wrong at the price of one slow iteration)
};

__device__ __forceinline__ long long means_wave_sum(long long v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the wave's registers into the workgroup's LDS record: s_all / s_msk point at the two sums' words
// (MASKED = false: one value stream into one pft_xsum -- no masked sum, s_msk is not touched; f12)
template <bool MASKED = true>
__device__ __forceinline__ void means_flush(MeansPair& st, int lane, unsigned long long* s_all, unsigned long long* s_msk)
{
  const long long a0 = means_wave_sum(st.a0), a1 = means_wave_sum(st.a1), a2 = means_wave_sum(st.a2);
  const long long m0 = MASKED ? means_wave_sum(st.m0) : 0, m1 = MASKED ? means_wave_sum(st.m1) : 0,
                  m2 = MASKED ? means_wave_sum(st.m2) : 0;
  if (lane == 0) {
    if (a0) atomicAdd(&s_all[st.cur], (unsigned long long)a0);
    if (a1) atomicAdd(&s_all[st.cur + 1], (unsigned long long)a1);
    if (a2) atomicAdd(&s_all[st.cur + 2], (unsigned long long)a2);
    if (MASKED) {
      if (m0) atomicAdd(&s_msk[st.cur], (unsigned long long)m0);
      if (m1) atomicAdd(&s_msk[st.cur + 1], (unsigned long long)m1);
      if (m2) atomicAdd(&s_msk[st.cur + 2], (unsigned long long)m2);
    }
  }
  st.a0 = st.a1 = st.a2 = st.m0 = st.m1 = st.m2 = 0;
}

// the three 32-bit digits of |x| (zero unless act) and its sign
__device__ __forceinline__ void means_digits(double x, bool act, unsigned& e0, unsigned& e1, unsigned& e2, bool& neg)
{
  const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
  const int E = (int)(bits >> 52) & 0x7ff;
  const unsigned long long M = (bits & 0xfffffffffffffULL) | (E ? 1ULL << 52 : 0ULL);
  const int s = ((E > 1 ? E : 1) - 1) & 31;
  const unsigned long long lo = act ? M << s : 0ULL;                    // T = M << s = hi * 2^64 + lo
  const unsigned long long hi = act ? (M >> 32) >> (32 - s) : 0ULL;     // (32 - s is 1..32; below 2^20)
  e0 = (unsigned)lo, e1 = (unsigned)(lo >> 32), e2 = (unsigned)hi;
  neg = (bits >> 63) != 0;
}

// the same as signed 64-bit integers
__device__ __forceinline__ void means_signed_digits(double x, bool act, long long& d0, long long& d1, long long& d2)
{
  unsigned e0, e1, e2;
  bool neg;
  means_digits(x, act, e0, e1, e2, neg);
  d0 = neg ? -(long long)e0 : (long long)e0, d1 = neg ? -(long long)e1 : (long long)e1;
  d2 = neg ? -(long long)e2 : (long long)e2;
}

// the eight values x[] of a wave's iteration (v: the slot exists, msk: it enters the masked sum)
// into st; n_all / n_msk: the wave-uniform counts of the cells that entered.  MASKED = false: the
// one-stream form of f12 -- msk, n_msk and s_msk are ignored and the m registers stay zero
template <int NE, int I0, int I1, bool MASKED = true>
__device__ __forceinline__ void means_accumulate(MeansPair& st, const double (&x)[NE], const bool (&v)[NE],
                                                 const bool (&msk)[NE], unsigned long long& n_all,
                                                 unsigned long long& n_msk, int lane, unsigned long long* s_all,
                                                 unsigned long long* s_msk)
{
  int c[NE];
  bool act[NE];
  bool other = false, minus = false;
#pragma unroll
  for (int i = I0; i < I1; ++i) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(x[i]);
    const int E = (int)(bits >> 52) & 0x7ff;
    const bool fin = v[i] && E != 0x7ff;
    act[i] = fin && (bits << 1) != 0;            // finite and not +-0
    c[i] = ((E > 1 ? E : 1) - 1) >> 5;
    n_all += __popcll(__ballot(fin));
    if (MASKED) n_msk += __popcll(__ballot(fin && msk[i]));
    other |= act[i] && c[i] != st.cur;
    minus |= act[i] && (bits >> 63) != 0;
  }
  const bool any_other = __ballot(other) != 0, any_minus = __ballot(minus) != 0;
  if (!any_other && !any_minus) {
    // every active lane of every slot is at cur and positive (u in kelvin, p in [0, 1]): the
    // digits are added as they are, 32-bit values into the 64-bit registers
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      unsigned e0, e1, e2;
      bool neg;
      means_digits(x[i], act[i], e0, e1, e2, neg);
      st.a0 += e0, st.a1 += e1, st.a2 += e2;
      if (MASKED) st.m0 += msk[i] ? e0 : 0u, st.m1 += msk[i] ? e1 : 0u, st.m2 += msk[i] ? e2 : 0u;
    }
    return;
  }
  if (!any_other) {
    // every active lane of every slot is at cur, some are negative
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      long long d0, d1, d2;
      means_signed_digits(x[i], act[i], d0, d1, d2);
      st.a0 += d0, st.a1 += d1, st.a2 += d2;
      if (MASKED) st.m0 += msk[i] ? d0 : 0, st.m1 += msk[i] ? d1 : 0, st.m2 += msk[i] ? d2 : 0;
    }
    return;
  }
#pragma unroll
  for (int i = I0; i < I1; ++i) {
    const unsigned long long m_act = __ballot(act[i]);
    if (!m_act) continue;
    if (!__ballot(act[i] && c[i] == st.cur)) {
      means_flush<MASKED>(st, lane, s_all, s_msk);
      st.cur = __builtin_amdgcn_readfirstlane(__shfl(c[i], (int)__ffsll((long long)m_act) - 1, 64));
    }
    long long d0, d1, d2;
    means_signed_digits(x[i], act[i], d0, d1, d2);
    const bool here = c[i] == st.cur;            // (inactive lanes: zero digits, either way nothing)
    st.a0 += here ? d0 : 0, st.a1 += here ? d1 : 0, st.a2 += here ? d2 : 0;
    if (MASKED) st.m0 += here && msk[i] ? d0 : 0, st.m1 += here && msk[i] ? d1 : 0, st.m2 += here && msk[i] ? d2 : 0;
    if (act[i] && !here) {
      if (d0) atomicAdd(&s_all[c[i]], (unsigned long long)d0);
      if (d1) atomicAdd(&s_all[c[i] + 1], (unsigned long long)d1);
      if (d2) atomicAdd(&s_all[c[i] + 2], (unsigned long long)d2);
      if (MASKED && msk[i]) {
        if (d0) atomicAdd(&s_msk[c[i]], (unsigned long long)d0);
        if (d1) atomicAdd(&s_msk[c[i] + 1], (unsigned long long)d1);
        if (d2) atomicAdd(&s_msk[c[i] + 2], (unsigned long long)d2);
      }
    }
  }
}

// A work item (f6, f12, f13: segment j of interior plane k, item = k * segs + j) and its pair-aligned
// frame: elements r = 0 .. span - 1 stand for e_base + r of the run of n3 planes, e_base on a 16-byte
// boundary at or one below the item's first element; of them [r_lo, r_hi) are the item's (nothing
// else is read), element r_lo being element `first` of the plane
struct ItemFrame {
  long e_base;
  int k, first, r_lo, r_hi, span;
};

__device__ __forceinline__ ItemFrame item_frame(long item, int segs, int seg_len, int plane, int head)
{
  ItemFrame f;
  f.k = (int)(item / segs);
  const int j = (int)(item - (long)f.k * segs);
  f.first = j * seg_len;                                            // within the plane
  const int len = plane - f.first < seg_len ? plane - f.first : seg_len;
  const long a = (long)f.k * plane + f.first;                       // within the run of n3 planes
  f.e_base = 2 * ((a + head) >> 1) - head;
  f.r_lo = (int)(a - f.e_base), f.r_hi = f.r_lo + len;
  f.span = (f.r_hi + 1) & ~1;
  return f;
}

struct MeansState {
  MeansPair u, p;
  unsigned long long n_u, n_p, n_ui, n_pp;   // wave-uniform counts
};

// one iteration of a wave: elements r0 .. r0 + 511 of the item's pair-aligned frame (of them
// [r_lo, r_hi) belong to the item; FULL: all do).  fu/fp/fg point at the frame's element 0.
template <bool FULL>
__device__ __forceinline__ void means_iter(MeansState& st, const double* __restrict__ fu, const double* __restrict__ fp,
                                           const double* __restrict__ fg, int r0, int r_lo, int r_hi, int lane,
                                           double p_thr, double gl_thr, unsigned long long* s_rec)
{
  constexpr int NE = 2 * PFT_DIAG_UNROLL;
  double u[NE], p[NE], g[NE];
  bool v[NE], ice[NE], pore[NE];
#pragma unroll
  for (int j = 0; j < PFT_DIAG_UNROLL; ++j) {
    const int r = r0 + 128 * j + 2 * lane;
    if (FULL) {
      const double2 a = *reinterpret_cast<const double2*>(fu + r);
      const double2 b = *reinterpret_cast<const double2*>(fp + r);
      const double2 c = *reinterpret_cast<const double2*>(fg + r);
      u[2 * j] = a.x, u[2 * j + 1] = a.y, p[2 * j] = b.x, p[2 * j + 1] = b.y, g[2 * j] = c.x, g[2 * j + 1] = c.y;
      v[2 * j] = v[2 * j + 1] = true;
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool ok = r + i >= r_lo && r + i < r_hi;
        v[2 * j + i] = ok;
        u[2 * j + i] = ok ? fu[r + i] : 0.0;
        p[2 * j + i] = ok ? fp[r + i] : 0.0;
        g[2 * j + i] = ok ? fg[r + i] : 0.0;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    // ordered comparisons: false on NaN
    ice[i] = v[i] && p[i] > p_thr;
    pore[i] = v[i] && g[i] < gl_thr;
  }
  unsigned long long* sums = s_rec + PFT_MEAN_COUNT;
  // (in two halves: fewer lane masks alive at a time)
  means_accumulate<NE, 0, NE / 2>(st.u, u, v, ice, st.n_u, st.n_ui, lane, sums + PFT_MEAN_U * PFT_XSUM_WORDS,
                                  sums + PFT_MEAN_U_ICE * PFT_XSUM_WORDS);
  means_accumulate<NE, 0, NE / 2>(st.p, p, v, pore, st.n_p, st.n_pp, lane, sums + PFT_MEAN_P * PFT_XSUM_WORDS,
                                  sums + PFT_MEAN_P_PORE * PFT_XSUM_WORDS);
  means_accumulate<NE, NE / 2, NE>(st.u, u, v, ice, st.n_u, st.n_ui, lane, sums + PFT_MEAN_U * PFT_XSUM_WORDS,
                                   sums + PFT_MEAN_U_ICE * PFT_XSUM_WORDS);
  means_accumulate<NE, NE / 2, NE>(st.p, p, v, pore, st.n_p, st.n_pp, lane, sums + PFT_MEAN_P * PFT_XSUM_WORDS,
                                   sums + PFT_MEAN_P_PORE * PFT_XSUM_WORDS);
}

// rec: the slab's record (written by means_total_kernel), then one record per interior plane
__global__ __launch_bounds__(PFT_DBLOCK) void means_kernel(const double* __restrict__ fu, const double* __restrict__ fp,
                                                           const double* __restrict__ fg, int plane, int head, int n3,
                                                           int segs, int seg_len, double p_thr, double gl_thr,
                                                           unsigned long long* __restrict__ rec)
{
  __shared__ unsigned long long s_rec[PFT_MEANS_REC];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int i = threadIdx.x; i < PFT_MEANS_REC; i += PFT_DBLOCK) s_rec[i] = 0;
  __syncthreads();
  MeansState st;
  st.u.a0 = st.u.a1 = st.u.a2 = st.u.m0 = st.u.m1 = st.u.m2 = 0;
  st.p.a0 = st.p.a1 = st.p.a2 = st.p.m0 = st.p.m1 = st.p.m2 = 0;
  st.u.cur = 32;
  st.p.cur = 31;
  const long items = (long)n3 * segs;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const ItemFrame it = item_frame(item, segs, seg_len, plane, head);
    const int k = it.k, r_lo = it.r_lo, r_hi = it.r_hi, span = it.span;
    const double* wu = fu + it.e_base;   // (e_base = -1: one before the run, never read at r = 0)
    const double* wp = fp + it.e_base;
    const double* wg = fg + it.e_base;
    st.n_u = st.n_p = st.n_ui = st.n_pp = 0;
    for (int r0 = PFT_DIAG_WAVE_ELEMS * wave; r0 < span; r0 += PFT_DIAG_WAVE_ELEMS * (PFT_DBLOCK / 64)) {
      if (r0 >= r_lo && r0 + PFT_DIAG_WAVE_ELEMS <= r_hi)
        means_iter<true>(st, wu, wp, wg, r0, r_lo, r_hi, lane, p_thr, gl_thr, s_rec);
      else
        means_iter<false>(st, wu, wp, wg, r0, r_lo, r_hi, lane, p_thr, gl_thr, s_rec);
    }
    unsigned long long* sums = s_rec + PFT_MEAN_COUNT;
    means_flush(st.u, lane, sums + PFT_MEAN_U * PFT_XSUM_WORDS, sums + PFT_MEAN_U_ICE * PFT_XSUM_WORDS);
    means_flush(st.p, lane, sums + PFT_MEAN_P * PFT_XSUM_WORDS, sums + PFT_MEAN_P_PORE * PFT_XSUM_WORDS);
    if (lane == 0) {
      if (st.n_u) atomicAdd(&s_rec[PFT_MEAN_U], st.n_u);
      if (st.n_p) atomicAdd(&s_rec[PFT_MEAN_P], st.n_p);
      if (st.n_ui) atomicAdd(&s_rec[PFT_MEAN_U_ICE], st.n_ui);
      if (st.n_pp) atomicAdd(&s_rec[PFT_MEAN_P_PORE], st.n_pp);
    }
    __syncthreads();
    // one thread per word: the non-zero ones to the plane's record, and the LDS copy zeroed again
    unsigned long long* dst = rec + (size_t)(k + 1) * PFT_MEANS_REC;
    for (int i = threadIdx.x; i < PFT_MEANS_REC; i += PFT_DBLOCK) {
      const unsigned long long x = s_rec[i];
      if (x) {
        atomicAdd(&dst[i], x);
        s_rec[i] = 0;
      }
    }
    __syncthreads();
  }
}

// the slab's record = the word-wise sum of the planes': per word four threads, each a quarter of
// the planes, then one of them stores the sum (no atomics: nobody else writes record 0)
__global__ __launch_bounds__(256) void means_total_kernel(unsigned long long* __restrict__ rec, int n3)
{
  __shared__ unsigned long long s_part[4][64];
  const int l = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int w = blockIdx.x * 64 + l;
  unsigned long long x = 0;
  if (w < PFT_MEANS_REC)
    for (int k = q; k < n3; k += 4) x += rec[(size_t)(k + 1) * PFT_MEANS_REC + w];
  s_part[q][l] = x;
  __syncthreads();
  if (q == 0 && w < PFT_MEANS_REC) rec[w] = s_part[0][l] + s_part[1][l] + s_part[2][l] + s_part[3][l];
}

extern "C" {

int pft_slab_means(pft_slab* s, int buf, const pft_diag_opts* opts, pft_means* total, pft_means* per_plane)
{
  if (!s || !total || buf < 0 || buf >= PFT_BUF_COUNT) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_means");
  const long plane = s->plane, n = (long)s->d.n3 * plane;
  // (a 64-bit word holds 2^31 digits; the kernel's 32-bit indices within a plane)
  if (n > 0x7fffffffL || plane > PFT_MEANS_MAX_PLANE) return -2;
  const size_t bytes = sizeof(pft_means) * ((size_t)s->d.n3 + 1);
  if (!s->means_dev) HIPCHK(hipMalloc((void**)&s->means_dev, bytes));
  if (!s->means_host) HIPCHK(hipHostMalloc((void**)&s->means_host, bytes, hipHostMallocDefault));
  int head, segs, seg_len;
  unsigned wgs;
  const double* fu = slab_fields(s, buf, &head);
  plane_work_cut(s, &segs, &seg_len, &wgs);
  const double p_thr = opts ? opts->p_thr : 0.5, gl_thr = opts ? opts->gl_thr : 0.5;
  // no state carries over between calls: every accumulator word is zeroed on the stream first
  HIPCHK(hipMemsetAsync(s->means_dev, 0, bytes, s->stream));
  if (s->means_timing) HIPCHK(hipEventRecord(s->ev_means[0], s->stream));
  means_kernel<<<wgs, PFT_DBLOCK, 0, s->stream>>>(fu, fu + s->fs, fu + 2 * s->fs, (int)plane, head, s->d.n3, segs, seg_len,
                                                  p_thr, gl_thr, s->means_dev);
  HIPCHK(hipGetLastError());
  means_total_kernel<<<(PFT_MEANS_REC + 63) / 64, 256, 0, s->stream>>>(s->means_dev, s->d.n3);
  HIPCHK(hipGetLastError());
  if (s->means_timing) HIPCHK(hipEventRecord(s->ev_means[1], s->stream));
  const size_t back = per_plane ? bytes : sizeof(pft_means);
  HIPCHK(hipMemcpyAsync(s->means_host, s->means_dev, back, hipMemcpyDeviceToHost, s->stream));
  const int rc = slab_wait(s, nullptr, "pft_slab_means");
  if (rc) return rc;
  memcpy(total, s->means_host, sizeof(pft_means));
  if (per_plane) memcpy(per_plane, s->means_host + PFT_MEANS_REC, sizeof(pft_means) * (size_t)s->d.n3);
  return 0;
}

int pft_slab_means_timing(pft_slab* s, int on) { return slab_timing_set(s, &pft_slab::means_timing, &pft_slab::ev_means, on); }

int pft_slab_means_last_ms(pft_slab* s, double* ms) { return slab_timing_ms(s, &pft_slab::means_timing, &pft_slab::ev_means, ms); }

}  // extern "C"

// ------------------------------------------------------------------------------------------
// f12: formula diagnostics (pft_formula.h) -- means_kernel's traversal (work items are segments of
// one interior plane, 16-byte loads, per iteration a wave takes 512 consecutive elements), but the
// value of a cell comes from a compiled program (pft_formula_compile) that the wave interprets:
// the program counter, the operator codes, the constants and the table descriptors are
// wave-uniform and read through read-only kernel-argument pointers (scalar loads), the operators
// are those of csrc/pft_ic_ops.h -- the host's -- and the evaluation stack is a per-lane column in
// LDS, st[slot * 256 + tid] (15 slots, 30 KiB per workgroup, every lane its own bank pair), with
// the top of the stack in a register: a runtime-indexed double st[16] would live in scratch.
// blockIdx.y is the program; each program re-reads the state (a field it never pushes is not
// loaded).  The reductions are integers only: counts by ballot and popcount, min / max through
// diag_key and maxabs through the bits of |v| (64-bit integer atomic max), the sum through
// means_accumulate in its one-stream form -- formula values have any sign and exponent, so its
// signed and per-lane paths are the usual ones here.  A plane's record (FD_REC words) is gathered
// in LDS per work item and added to the plane's record in global memory; formula_total_kernel
// combines the planes' records into the slab's.
//
// No loop here depends on a cell's value but the factorial's, bounded at 170: C and P never reach
// the device (pft_formula_compile; pft_slab_formulas refuses them), and their loop is not even
// compiled into this file (PFT_IC_NO_CP above).  After a math error a lane goes on through the
// remaining entries -- the program counter is the wave's -- and yields 0 at the end, the value
// pft_ic_run returns at once.
enum { FD_N = 0, FD_NONZERO, FD_NONFINITE, FD_MAX, FD_MIN, FD_MAXABS, FD_SUM, FD_REC = FD_SUM + PFT_XSUM_WORDS };
#define PFT_FORMULA_SLOTS (PFT_IC_STACK - 1)   // LDS slots: the top of the stack is a register
enum { FM_NEED_U = 1, FM_NEED_P = 2, FM_NEED_GL = 4, FM_NEED_IJ = 8 };

// the programs of one call, all in one device blob.  code[c] = {op, aux}: 100 push arg[c]; 101 push
// the node's field aux (0 u, 1 p, 2 gl); 102 / 103 / 104 push entry aux + i / j / k of tval (its
// math-error flag in terr); the operators of pft_ic_ops.h.  meta[3 f ..]: program f's first entry,
// the entry past its last, its FM_NEED_* bits.
struct FormulaProgs {
  const int2* __restrict__ code;
  const double* __restrict__ arg;
  const double* __restrict__ tval;
  const unsigned char* __restrict__ terr;
  const int* __restrict__ meta;
};

// pft_ic_run's semantics at one node: entries [c0, c1), st this lane's LDS column
__device__ __forceinline__ double formula_eval(const FormulaProgs& P, int c0, int c1, double u, double p, double g,
                                               int i, int j, int k, double* st)
{
  double top = 0.0;
  int sp = 0, err = 0;
  for (int c = c0; c < c1; ++c) {
    const int2 cd = P.code[c];
    const int o = cd.x;
    if (o >= 100) {
      double v;
      if (o == 100)
        v = P.arg[c];
      else if (o == 101)
        v = cd.y == 0 ? u : (cd.y == 1 ? p : g);
      else {
        const int x = cd.y + (o == 102 ? i : (o == 103 ? j : k));
        err |= P.terr[x];
        v = P.tval[x];
      }
      if (sp > 0) st[(sp - 1) * PFT_DBLOCK] = top;
      top = v;
      ++sp;
    } else if (o < 20) {
      --sp;
      top = pft_ic_binary(o, st[(sp - 1) * PFT_DBLOCK], top, &err);
    } else {
      top = pft_ic_unary(o, top, &err);
    }
  }
  return err ? 0.0 : top;   // a math error anywhere yields 0, as the reference's Eval()
}

// the pair of elements r, r + 1 of the fields that `need` names (the others stay 0): one 16-byte load
// per field where both belong to the item (full), else each element alone under its own test
__device__ __forceinline__ void formula_load(bool full, int need, const double* __restrict__ fu,
                                             const double* __restrict__ fp, const double* __restrict__ fg, int r, int r_lo,
                                             int r_hi, double (&u)[2], double (&p)[2], double (&g)[2], bool (&v)[2])
{
  if (full) {
    if (need & FM_NEED_U) {
      const double2 a = *reinterpret_cast<const double2*>(fu + r);
      u[0] = a.x, u[1] = a.y;
    }
    if (need & FM_NEED_P) {
      const double2 a = *reinterpret_cast<const double2*>(fp + r);
      p[0] = a.x, p[1] = a.y;
    }
    if (need & FM_NEED_GL) {
      const double2 a = *reinterpret_cast<const double2*>(fg + r);
      g[0] = a.x, g[1] = a.y;
    }
    v[0] = v[1] = true;
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool ok = r + h >= r_lo && r + h < r_hi;
      v[h] = ok;
      if (ok && (need & FM_NEED_U)) u[h] = fu[r + h];
      if (ok && (need & FM_NEED_P)) p[h] = fp[r + h];
      if (ok && (need & FM_NEED_GL)) g[h] = fg[r + h];
    }
  }
}

struct FormulaState {
  MeansPair sum;
  unsigned long long n, nonzero, nonfinite;   // wave-uniform counts
  unsigned long long kmax, kmin, kabs;        // per-lane keys (0: no value yet)
};

// one iteration of a wave: elements r0 .. r0 + 511 of the item's pair-aligned frame (of them
// [r_lo, r_hi) belong to the item, element r_lo being element `first` of plane k; FULL: all do)
template <bool FULL>
__device__ __forceinline__ void formula_iter(FormulaState& st, const FormulaProgs& P, int c0, int c1, int need,
                                             const double* __restrict__ fu, const double* __restrict__ fp,
                                             const double* __restrict__ fg, int r0, int r_lo, int r_hi, int first,
                                             int n1, int k, int lane, double* stack, unsigned long long* s_sum)
{
#pragma unroll 1
  for (int jj = 0; jj < PFT_DIAG_UNROLL; ++jj) {
    const int r = r0 + 128 * jj + 2 * lane;
    double u[2] = {0.0, 0.0}, p[2] = {0.0, 0.0}, g[2] = {0.0, 0.0}, x[2];
    bool v[2];
    formula_load(FULL, need, fu, fp, fg, r, r_lo, r_hi, u, p, g, v);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // the node's place in its plane; a slot outside the item evaluates node 0 (inside every
      // table) and is left out of every count below
      const int e = v[h] ? first + (r + h - r_lo) : 0;
      int i = 0, j = 0;
      if (need & FM_NEED_IJ) {
        j = e / n1;
        i = e - j * n1;
      }
      x[h] = formula_eval(P, c0, c1, u[h], p[h], g[h], i, j, k, stack);
      st.nonzero += __popcll(__ballot(v[h] && x[h] != 0));          // (a NaN is "true")
      st.nonfinite += __popcll(__ballot(v[h] && !diag_finite(x[h])));
      if (v[h] && x[h] == x[h]) {
        const unsigned long long key = diag_key(x[h]);
        const unsigned long long a = (unsigned long long)__double_as_longlong(fabs(x[h]));
        st.kmax = key > st.kmax ? key : st.kmax;
        st.kmin = ~key > st.kmin ? ~key : st.kmin;
        st.kabs = a > st.kabs ? a : st.kabs;   // non-negative doubles (and +Inf) order as their bits
      }
    }
    unsigned long long unused = 0;
    means_accumulate<2, 0, 2, false>(st.sum, x, v, v, st.n, unused, lane, s_sum, s_sum);
  }
}

// rec: PFT_FORMULA_MAX total records (written by formula_total_kernel), then for program f the
// records of its n3 planes from record PFT_FORMULA_MAX + f * n3
__global__ __launch_bounds__(PFT_DBLOCK) void formula_kernel(const double* __restrict__ fu, const double* __restrict__ fp,
                                                             const double* __restrict__ fg, int plane, int head, int n1,
                                                             int n3, int segs, int seg_len, FormulaProgs P,
                                                             unsigned long long* __restrict__ rec)
{
  __shared__ double s_stack[PFT_FORMULA_SLOTS * PFT_DBLOCK];
  __shared__ unsigned long long s_rec[FD_REC];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int f = blockIdx.y;
  const int c0 = P.meta[3 * f], c1 = P.meta[3 * f + 1], need = P.meta[3 * f + 2];
  for (int i = threadIdx.x; i < FD_REC; i += PFT_DBLOCK) s_rec[i] = 0;
  __syncthreads();
  FormulaState st;
  st.sum.a0 = st.sum.a1 = st.sum.a2 = st.sum.m0 = st.sum.m1 = st.sum.m2 = 0;
  st.sum.cur = 32;
  double* stack = s_stack + threadIdx.x;
  unsigned long long* planes = rec + (size_t)(PFT_FORMULA_MAX + (size_t)f * n3) * FD_REC;
  const long items = (long)n3 * segs;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const ItemFrame it = item_frame(item, segs, seg_len, plane, head);
    const int k = it.k, first = it.first, r_lo = it.r_lo, r_hi = it.r_hi, span = it.span;
    const double* wu = fu + it.e_base;   // (e_base = -1: one before the run, never read at r = 0)
    const double* wp = fp + it.e_base;
    const double* wg = fg + it.e_base;
    st.n = st.nonzero = st.nonfinite = 0;
    st.kmax = st.kmin = st.kabs = 0;
    for (int r0 = PFT_DIAG_WAVE_ELEMS * wave; r0 < span; r0 += PFT_DIAG_WAVE_ELEMS * (PFT_DBLOCK / 64)) {
      if (r0 >= r_lo && r0 + PFT_DIAG_WAVE_ELEMS <= r_hi)
        formula_iter<true>(st, P, c0, c1, need, wu, wp, wg, r0, r_lo, r_hi, first, n1, k, lane, stack, s_rec + FD_SUM);
      else
        formula_iter<false>(st, P, c0, c1, need, wu, wp, wg, r0, r_lo, r_hi, first, n1, k, lane, stack, s_rec + FD_SUM);
    }
    means_flush<false>(st.sum, lane, s_rec + FD_SUM, s_rec + FD_SUM);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      unsigned long long o;
      o = __shfl_xor(st.kmax, off, 64), st.kmax = o > st.kmax ? o : st.kmax;
      o = __shfl_xor(st.kmin, off, 64), st.kmin = o > st.kmin ? o : st.kmin;
      o = __shfl_xor(st.kabs, off, 64), st.kabs = o > st.kabs ? o : st.kabs;
    }
    if (lane == 0) {
      if (st.n) atomicAdd(&s_rec[FD_N], st.n);
      if (st.nonzero) atomicAdd(&s_rec[FD_NONZERO], st.nonzero);
      if (st.nonfinite) atomicAdd(&s_rec[FD_NONFINITE], st.nonfinite);
      if (st.kmax) atomicMax(&s_rec[FD_MAX], st.kmax);
      if (st.kmin) atomicMax(&s_rec[FD_MIN], st.kmin);
      if (st.kabs) atomicMax(&s_rec[FD_MAXABS], st.kabs);
    }
    __syncthreads();
    // one thread per word: the non-zero ones to the plane's record, and the LDS copy zeroed again
    unsigned long long* dst = planes + (size_t)k * FD_REC;
    for (int i = threadIdx.x; i < FD_REC; i += PFT_DBLOCK) {
      const unsigned long long x = s_rec[i];
      if (x) {
        if (i >= FD_MAX && i <= FD_MAXABS)
          atomicMax(&dst[i], x);
        else
          atomicAdd(&dst[i], x);
        s_rec[i] = 0;
      }
    }
    __syncthreads();
  }
}

// program blockIdx.y's slab record = its planes' records combined word by word (counts and sum
// words add, keys take the maximum): per word four threads, each a quarter of the planes, then one
// of them stores the result (no atomics: nobody else writes the total records)
__global__ __launch_bounds__(256) void formula_total_kernel(unsigned long long* __restrict__ rec, int n3)
{
  __shared__ unsigned long long s_part[4][64];
  const int l = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int w = blockIdx.x * 64 + l, f = blockIdx.y;
  const bool is_key = w >= FD_MAX && w <= FD_MAXABS;
  const unsigned long long* planes = rec + (size_t)(PFT_FORMULA_MAX + (size_t)f * n3) * FD_REC;
  unsigned long long x = 0;
  if (w < FD_REC)
    for (int k = q; k < n3; k += 4) {
      const unsigned long long o = planes[(size_t)k * FD_REC + w];
      x = is_key ? (o > x ? o : x) : x + o;
    }
  s_part[q][l] = x;
  __syncthreads();
  if (q == 0 && w < FD_REC) {
    for (int i = 1; i < 4; ++i) {
      const unsigned long long o = s_part[i][l];
      x = is_key ? (o > x ? o : x) : x + o;
    }
    rec[(size_t)f * FD_REC + w] = x;
  }
}

// a device record's words as a pft_fdiag of `cells` cells
static void formula_record(const unsigned long long* h, long long cells, pft_fdiag* out)
{
  const double inf = __builtin_inf();
  out->cells = cells;
  out->n = (long long)h[FD_N];
  out->nonzero = (long long)h[FD_NONZERO];
  out->nonfinite = (long long)h[FD_NONFINITE];
  out->max = h[FD_MAX] ? diag_unkey(h[FD_MAX]) : -inf;
  out->min = h[FD_MIN] ? diag_unkey(~h[FD_MIN]) : inf;
  memcpy(&out->maxabs, &h[FD_MAXABS], 8);
  memcpy(out->sum.w, h + FD_SUM, sizeof(out->sum.w));
}

// The programs of one call (f12: up to PFT_FORMULA_MAX; f13: the value and the mask) checked
// before anything is launched: only what the device runs exactly and in bounded time (else 1: not
// device-exact), a stack within the LDS column (else 1), a well-formed program with tables of this
// slab's grid (else -2).  entries / tvals: the programs' entries and table values together.
static int formula_progs_check(const pft_slab* s, int nprog, const pft_ic_prog* const* progs, long* entries_out,
                               long* tvals_out)
{
  long entries = 0, tvals = 0;
  bool inexact = false;
  for (int f = 0; f < nprog; ++f) {
    const pft_ic_prog* p = progs[f];
    if (p->n < 1 || !p->op || !p->arg || p->ntab < 0 || (p->ntab > 0 && (!p->tab_axis || !p->tab_off || !p->tab_val || !p->tab_err)))
      return -2;
    int depth = 0;
    for (int c = 0; c < p->n; ++c) {
      const int o = p->op[c];
      if (o == 100)
        ++depth;
      else if (o == 101) {
        if (p->arg[c] != 6.0 && p->arg[c] != 7.0 && p->arg[c] != 8.0) return -2;
        ++depth;
      } else if (o == 102) {
        const double t = p->arg[c];
        if (!(t >= 0 && t < p->ntab) || t != (double)(int)t) return -2;
        ++depth;
      } else if (!((o >= 1 && o <= 15) || (o >= 20 && o <= 48)))
        return -2;
      else {
        if (o == 5 || o == 6 || !pft_ic_op_device(o)) inexact = true;
        if (o < 20) --depth;
      }
      if (depth < 1) return -2;
      if (depth > PFT_IC_STACK) inexact = true;
    }
    if (depth != 1) return -2;
    for (int t = 0; t < p->ntab; ++t) {
      const int ax = p->tab_axis[t];
      const long len = (t + 1 < p->ntab ? p->tab_off[t + 1] : p->tab_len) - p->tab_off[t];
      if (ax < 0 || ax > 2 || p->tab_off[t] < 0 || len != (ax == 0 ? s->d.n1 : (ax == 1 ? s->d.n2 : s->d.n3))) return -2;
    }
    entries += p->n;
    tvals += p->ntab > 0 ? p->tab_len : 0;
  }
  if (entries > PFT_FORMULA_MAX_ENTRIES || tvals > 0x7fffffffL) return -2;
  *entries_out = entries, *tvals_out = tvals;
  return inexact ? 1 : 0;
}

// The checked programs packed into the slab's pinned blob, [arg][tval][code][meta][terr][extra]
// (grown on demand, device and host): P points at the device copy's parts, *extra_dev at `extra`
// bytes behind them on an 8-byte boundary (copied from extra_src: f13's edges), *bytes is what the
// caller copies to the device on its stream.
static int formula_progs_pack(pft_slab* s, int nprog, const pft_ic_prog* const* progs, long entries, long tvals,
                              size_t extra, const void* extra_src, FormulaProgs* P, const char** extra_dev, size_t* bytes)
{
  const size_t nv = (size_t)(tvals > 0 ? tvals : 1);
  const size_t o_arg = 0, o_val = o_arg + sizeof(double) * (size_t)entries, o_code = o_val + sizeof(double) * nv,
               o_meta = o_code + sizeof(int2) * (size_t)entries, o_err = o_meta + sizeof(int) * 3 * PFT_FORMULA_MAX,
               o_extra = (o_err + nv + 7) & ~(size_t)7, blob = extra ? o_extra + extra : o_err + nv;
  if (blob > s->formula_prog_cap) {
    const size_t cap = 2 * blob;
    if (s->formula_prog_dev) HIPCHK(hipFree(s->formula_prog_dev));
    if (s->formula_prog_host) HIPCHK(hipHostFree(s->formula_prog_host));
    s->formula_prog_dev = s->formula_prog_host = nullptr;
    s->formula_prog_cap = 0;
    HIPCHK(hipMalloc((void**)&s->formula_prog_dev, cap));
    HIPCHK(hipHostMalloc((void**)&s->formula_prog_host, cap, hipHostMallocDefault));
    s->formula_prog_cap = cap;
  }
  char* h = s->formula_prog_host;
  double* h_arg = (double*)(h + o_arg);
  double* h_val = (double*)(h + o_val);
  int2* h_code = (int2*)(h + o_code);
  int* h_meta = (int*)(h + o_meta);
  unsigned char* h_err = (unsigned char*)(h + o_err);
  long c_at = 0, v_at = 0;
  h_val[0] = 0.0, h_err[0] = 0;
  for (int f = 0; f < nprog; ++f) {
    const pft_ic_prog* p = progs[f];
    int need = 0;
    h_meta[3 * f] = (int)c_at;
    for (int c = 0; c < p->n; ++c, ++c_at) {
      const int o = p->op[c];
      h_arg[c_at] = p->arg[c];
      h_code[c_at] = make_int2(o, 0);
      if (o == 101) {
        const int q = (int)p->arg[c] - 6;
        h_code[c_at].y = q;
        need |= 1 << q;
      } else if (o == 102) {
        const int t = (int)p->arg[c], ax = p->tab_axis[t];
        h_code[c_at] = make_int2(102 + ax, (int)(v_at + p->tab_off[t]));
        if (ax < 2) need |= FM_NEED_IJ;
      }
    }
    h_meta[3 * f + 1] = (int)c_at;
    h_meta[3 * f + 2] = need;
    if (p->ntab > 0) {
      memcpy(h_val + v_at, p->tab_val, sizeof(double) * (size_t)p->tab_len);
      memcpy(h_err + v_at, p->tab_err, (size_t)p->tab_len);
      v_at += p->tab_len;
    }
  }
  if (extra) memcpy(h + o_extra, extra_src, extra);
  P->arg = (const double*)(s->formula_prog_dev + o_arg);
  P->tval = (const double*)(s->formula_prog_dev + o_val);
  P->code = (const int2*)(s->formula_prog_dev + o_code);
  P->meta = (const int*)(s->formula_prog_dev + o_meta);
  P->terr = (const unsigned char*)(s->formula_prog_dev + o_err);
  if (extra_dev) *extra_dev = s->formula_prog_dev + o_extra;
  *bytes = blob;
  return 0;
}

extern "C" {

int pft_slab_formulas(pft_slab* s, int buf, int nprog, const pft_ic_prog* progs, pft_fdiag* total, pft_fdiag* per_plane)
{
  if (!s || !progs || !total || buf < 0 || buf >= PFT_BUF_COUNT || nprog < 1 || nprog > PFT_FORMULA_MAX) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_formulas");
  const long plane = s->plane, n = (long)s->d.n3 * plane;
  const int n3 = s->d.n3;
  if (n > 0x7fffffffL || plane > PFT_MEANS_MAX_PLANE) return -2;
  const pft_ic_prog* list[PFT_FORMULA_MAX];
  for (int f = 0; f < nprog; ++f) list[f] = &progs[f];
  long entries = 0, tvals = 0;
  int rc_pack = formula_progs_check(s, nprog, list, &entries, &tvals);
  if (rc_pack) return rc_pack;
  FormulaProgs P;
  size_t blob = 0;
  if ((rc_pack = formula_progs_pack(s, nprog, list, entries, tvals, 0, nullptr, &P, nullptr, &blob))) return rc_pack;
  const size_t words = (size_t)FD_REC * (PFT_FORMULA_MAX + (size_t)PFT_FORMULA_MAX * n3);
  if (!s->formula_dev) HIPCHK(hipMalloc((void**)&s->formula_dev, sizeof(unsigned long long) * words));
  if (!s->formula_host) HIPCHK(hipHostMalloc((void**)&s->formula_host, sizeof(unsigned long long) * words, hipHostMallocDefault));
  int head, segs, seg_len;
  unsigned wgs;   // (the cap holds per program)
  const double* fu = slab_fields(s, buf, &head);
  plane_work_cut(s, &segs, &seg_len, &wgs);
  const size_t used = sizeof(unsigned long long) * FD_REC * (PFT_FORMULA_MAX + (size_t)nprog * n3);
  HIPCHK(hipMemcpyAsync(s->formula_prog_dev, s->formula_prog_host, blob, hipMemcpyHostToDevice, s->stream));
  // no state carries over between calls: every accumulator word is zeroed on the stream first
  HIPCHK(hipMemsetAsync(s->formula_dev, 0, used, s->stream));
  if (s->formula_timing) HIPCHK(hipEventRecord(s->ev_formula[0], s->stream));
  formula_kernel<<<dim3(wgs, (unsigned)nprog), PFT_DBLOCK, 0, s->stream>>>(fu, fu + s->fs, fu + 2 * s->fs, (int)plane, head,
                                                                           s->d.n1, n3, segs, seg_len, P, s->formula_dev);
  HIPCHK(hipGetLastError());
  formula_total_kernel<<<dim3((FD_REC + 63) / 64, (unsigned)nprog), 256, 0, s->stream>>>(s->formula_dev, n3);
  HIPCHK(hipGetLastError());
  if (s->formula_timing) HIPCHK(hipEventRecord(s->ev_formula[1], s->stream));
  const size_t back = per_plane ? used : sizeof(unsigned long long) * FD_REC * (size_t)nprog;
  HIPCHK(hipMemcpyAsync(s->formula_host, s->formula_dev, back, hipMemcpyDeviceToHost, s->stream));
  const int rc = slab_wait(s, nullptr, "pft_slab_formulas");
  if (rc) return rc;
  for (int f = 0; f < nprog; ++f) {
    formula_record(s->formula_host + (size_t)f * FD_REC, n, &total[f]);
    if (per_plane)
      for (int k = 0; k < n3; ++k)
        formula_record(s->formula_host + (size_t)(PFT_FORMULA_MAX + (size_t)f * n3 + k) * FD_REC, plane,
                       &per_plane[(size_t)f * n3 + k]);
  }
  return 0;
}

int pft_slab_formulas_timing(pft_slab* s, int on) { return slab_timing_set(s, &pft_slab::formula_timing, &pft_slab::ev_formula, on); }

int pft_slab_formulas_last_ms(pft_slab* s, double* ms) { return slab_timing_ms(s, &pft_slab::formula_timing, &pft_slab::ev_formula, ms); }

}  // extern "C"

// ------------------------------------------------------------------------------------------
// f13: histograms of formula values (pft_hist.h) -- formula_kernel's traversal and interpreter, but
// what is reduced is a count per bin.  Program 0 of the blob is the value, program 1 (when there is
// one) the mask; a cell's mask and then its value are evaluated by formula_eval on the same LDS
// stack column, with the wave's program counter: unselected lanes run along and are left out of
// every count.  The edges are copied into LDS once per workgroup; a selected value's bin is the
// number of edges <= v, less one, found by a binary search without branches whose trip count
// `trips` = ceil(log2(nbins + 1)) is a kernel argument -- no loop depends on a cell's value.
//
// Counts are integers only.  selected / nan / under / over go by ballot and popcount in scalar
// registers.  Bin counts go to 32-bit LDS counters (an item is at most a plane, <= 2^30 cells).
// The usual state of this model has almost every cell in one bin (u = 293.15 over most of the
// domain, p at 0 or 1), so a wave first aggregates equal bins: PFT_HIST_ROUNDS times (once: measured) it takes the
// bin of its first remaining lane, ballots the lanes that share it and lets that lane add the
// popcount; the lanes still left add 1 each (ds_add_u32).  At the end of an item one thread per
// non-zero word adds it to the plane's row in global memory (64-bit integer atomicAdd) and zeroes
// the LDS word; hist_total_kernel adds the planes' rows into the slab's.  No floating-point
// atomic, no compare-and-swap, no spin.
//
// LDS: 30 720 (stack) + 8 200 (edges) + 4 096 (counters) + 32 (head) bytes.
#ifndef PFT_HIST_ROUNDS
#define PFT_HIST_ROUNDS 1   // (scripts/hist_time.py on builds with 0, 1, 2 and 4: DESIGN.md section 7, f13)
#endif
enum { HD_SELECTED = 0, HD_NAN, HD_UNDER, HD_OVER, HD_WORDS };

struct HistState {
  unsigned long long selected, nan, under, over;   // wave-uniform counts
};

// one iteration of a wave, as formula_iter (full: every slot of the 512 belongs to the item): c0..c1
// the value's entries, m0..m1 the mask's (m0 == m1: no mask), need the fields and indices either
// program pushes.  The interpreter is compiled into the kernel once: the full and the ragged
// iteration differ in their loads only, and the two elements of a pair and the two programs take
// turns through the same copy (loops that are not unrolled) -- eight inlined copies are more code
// than the instruction cache holds.
__device__ __forceinline__ void hist_iter(HistState& st, const FormulaProgs& P, int c0, int c1, int m0, int m1, int need,
                                          bool full, const double* __restrict__ fu, const double* __restrict__ fp,
                                          const double* __restrict__ fg, int r0, int r_lo, int r_hi, int first,
                                          int n1, int k, int lane, double* stack, const double* s_edges,
                                          unsigned* s_cnt, int nbins, int trips, double e_first, double e_last)
{
#pragma unroll 1
  for (int jj = 0; jj < PFT_DIAG_UNROLL; ++jj) {
    const int r = r0 + 128 * jj + 2 * lane;
    double u[2] = {0.0, 0.0}, p[2] = {0.0, 0.0}, g[2] = {0.0, 0.0};
    bool v[2];
    formula_load(full, need, fu, fp, fg, r, r_lo, r_hi, u, p, g, v);
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const double uh = h ? u[1] : u[0], ph = h ? p[1] : p[0], gh = h ? g[1] : g[0];
      const bool vh = h ? v[1] : v[0];
      // the node's place in its plane; a slot outside the item evaluates node 0 (inside every
      // table) and is left out of every count below
      const int e = vh ? first + (r + h - r_lo) : 0;
      int i = 0, j = 0;
      if (need & FM_NEED_IJ) {
        j = e / n1;
        i = e - j * n1;
      }
      bool sel = vh;
      double x = 0.0;
#pragma unroll 1
      for (int pass = m1 > m0 ? 0 : 1; pass < 2; ++pass) {
        const double val = formula_eval(P, pass ? c0 : m0, pass ? c1 : m1, uh, ph, gh, i, j, k, stack);
        if (pass == 0)
          sel = sel && val != 0;   // (a NaN is "true")
        else
          x = val;
      }
      // pos: the number of edges <= x (0 for a NaN); every lane makes the same `trips` steps
      int pos = 0;
      // (index clamped and both tests combined bitwise: one ds_read_b64, compares and a shift per
      // step, no exec-mask branch)
      for (int t = trips - 1; t >= 0; --t) {
        const int at = pos + (1 << t) - 1;
        const double ed = s_edges[at < nbins ? at : nbins];
        pos += (int)((unsigned)(at <= nbins) & (unsigned)(ed <= x)) << t;
      }
      const bool is_nan = sel && x != x, is_under = sel && x < e_first, is_over = sel && x > e_last;
      const bool binned = sel && x >= e_first && x <= e_last;      // (ordered: false on NaN)
      const int b = pos > nbins ? nbins - 1 : pos - 1;             // x == the last edge: the last bin
      st.selected += __popcll(__ballot(sel));
      st.nan += __popcll(__ballot(is_nan));
      st.under += __popcll(__ballot(is_under));
      st.over += __popcll(__ballot(is_over));
      unsigned long long rem = __ballot(binned);
#pragma unroll
      for (int round = 0; round < PFT_HIST_ROUNDS; ++round) {
        if (!rem) break;
        const int lead = (int)__ffsll((long long)rem) - 1;
        const int lb = __builtin_amdgcn_readlane(b, lead);
        const unsigned long long same = __ballot(binned && b == lb) & rem;
        if (lane == lead) atomicAdd(&s_cnt[lb], (unsigned)__popcll(same));
        rem &= ~same;
      }
      if ((rem >> lane) & 1) atomicAdd(&s_cnt[b], 1u);
    }
  }
}

// rec: rows of `row` = HD_WORDS + nbins words: row 0 the slab's (written by hist_total_kernel), row
// 1 + k interior plane k's
__global__ __launch_bounds__(PFT_DBLOCK) void hist_kernel(const double* __restrict__ fu, const double* __restrict__ fp,
                                                          const double* __restrict__ fg, int plane, int head, int n1,
                                                          int n3, int segs, int seg_len, FormulaProgs P, int has_mask,
                                                          const double* __restrict__ edges, int nbins, int trips,
                                                          unsigned long long* __restrict__ rec)
{
  __shared__ double s_stack[PFT_FORMULA_SLOTS * PFT_DBLOCK];
  __shared__ double s_edges[PFT_HIST_MAX_BINS + 1];
  __shared__ unsigned s_cnt[PFT_HIST_MAX_BINS];
  __shared__ unsigned long long s_head[HD_WORDS];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c0 = P.meta[0], c1 = P.meta[1];
  const int m0 = has_mask ? P.meta[3] : 0, m1 = has_mask ? P.meta[4] : 0;
  const int need = P.meta[2] | (has_mask ? P.meta[5] : 0);
  for (int i = threadIdx.x; i <= nbins; i += PFT_DBLOCK) s_edges[i] = edges[i];
  for (int i = threadIdx.x; i < nbins; i += PFT_DBLOCK) s_cnt[i] = 0;
  if (threadIdx.x < HD_WORDS) s_head[threadIdx.x] = 0;
  __syncthreads();
  const double e_first = s_edges[0], e_last = s_edges[nbins];
  const int row = HD_WORDS + nbins;
  HistState st;
  double* stack = s_stack + threadIdx.x;
  const long items = (long)n3 * segs;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const ItemFrame it = item_frame(item, segs, seg_len, plane, head);
    const int k = it.k, first = it.first, r_lo = it.r_lo, r_hi = it.r_hi, span = it.span;
    const double* wu = fu + it.e_base;   // (e_base = -1: one before the run, never read at r = 0)
    const double* wp = fp + it.e_base;
    const double* wg = fg + it.e_base;
    st.selected = st.nan = st.under = st.over = 0;
    for (int r0 = PFT_DIAG_WAVE_ELEMS * wave; r0 < span; r0 += PFT_DIAG_WAVE_ELEMS * (PFT_DBLOCK / 64)) {
      hist_iter(st, P, c0, c1, m0, m1, need, r0 >= r_lo && r0 + PFT_DIAG_WAVE_ELEMS <= r_hi, wu, wp, wg, r0, r_lo, r_hi,
                first, n1, k, lane, stack, s_edges, s_cnt, nbins, trips, e_first, e_last);
    }
    if (lane == 0) {
      if (st.selected) atomicAdd(&s_head[HD_SELECTED], st.selected);
      if (st.nan) atomicAdd(&s_head[HD_NAN], st.nan);
      if (st.under) atomicAdd(&s_head[HD_UNDER], st.under);
      if (st.over) atomicAdd(&s_head[HD_OVER], st.over);
    }
    __syncthreads();
    // one thread per word: the non-zero ones to the plane's row, and the LDS copy zeroed again
    unsigned long long* dst = rec + (size_t)(k + 1) * row;
    for (int i = threadIdx.x; i < row; i += PFT_DBLOCK) {
      if (i < HD_WORDS) {
        const unsigned long long x = s_head[i];
        if (x) {
          atomicAdd(&dst[i], x);
          s_head[i] = 0;
        }
      } else {
        const unsigned x = s_cnt[i - HD_WORDS];
        if (x) {
          atomicAdd(&dst[i], (unsigned long long)x);
          s_cnt[i - HD_WORDS] = 0;
        }
      }
    }
    __syncthreads();
  }
}

// the slab's row = the word-wise sum of the planes': per word four threads, each a quarter of the
// planes, then one of them stores the sum (no atomics: nobody else writes row 0)
__global__ __launch_bounds__(256) void hist_total_kernel(unsigned long long* __restrict__ rec, int n3, int row)
{
  __shared__ unsigned long long s_part[4][64];
  const int l = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int w = blockIdx.x * 64 + l;
  unsigned long long x = 0;
  if (w < row)
    for (int k = q; k < n3; k += 4) x += rec[(size_t)(k + 1) * row + w];
  s_part[q][l] = x;
  __syncthreads();
  if (q == 0 && w < row) rec[w] = s_part[0][l] + s_part[1][l] + s_part[2][l] + s_part[3][l];
}

// a device row's words as a record of `cells` cells
static void hist_record(const unsigned long long* h, long long cells, int nbins, pft_hist_head* head, long long* counts)
{
  if (head) {
    head->cells = cells;
    head->selected = (long long)h[HD_SELECTED];
    head->nan = (long long)h[HD_NAN];
    head->under = (long long)h[HD_UNDER];
    head->over = (long long)h[HD_OVER];
  }
  if (counts) memcpy(counts, h + HD_WORDS, sizeof(long long) * (size_t)nbins);
}

extern "C" {

int pft_slab_hist(pft_slab* s, int buf, const pft_ic_prog* value_prog, const pft_ic_prog* mask_prog, int nbins,
                  const double* edges, pft_hist_head* head, long long* counts, pft_hist_head* plane_heads,
                  long long* plane_counts)
{
  if (!s || !value_prog || !head || !counts || buf < 0 || buf >= PFT_BUF_COUNT) return -2;
  if (pft_hist_check(nbins, edges)) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_hist");
  const long plane = s->plane, n = (long)s->d.n3 * plane;
  const int n3 = s->d.n3;
  if (n > 0x7fffffffL || plane > PFT_MEANS_MAX_PLANE) return -2;
  const pft_ic_prog* list[2] = {value_prog, mask_prog};
  const int nprog = mask_prog ? 2 : 1;
  long entries = 0, tvals = 0;
  int rc_pack = formula_progs_check(s, nprog, list, &entries, &tvals);
  if (rc_pack) return rc_pack;
  FormulaProgs P;
  const char* edges_dev = nullptr;
  size_t blob = 0;
  if ((rc_pack = formula_progs_pack(s, nprog, list, entries, tvals, sizeof(double) * ((size_t)nbins + 1), edges, &P,
                                    &edges_dev, &blob)))
    return rc_pack;
  const int row = HD_WORDS + nbins;
  const size_t bytes = sizeof(unsigned long long) * (size_t)row * ((size_t)n3 + 1);
  if (bytes > s->hist_cap) {
    if (s->hist_dev) HIPCHK(hipFree(s->hist_dev));
    if (s->hist_host) HIPCHK(hipHostFree(s->hist_host));
    s->hist_dev = s->hist_host = nullptr;
    s->hist_cap = 0;
    HIPCHK(hipMalloc((void**)&s->hist_dev, bytes));
    HIPCHK(hipHostMalloc((void**)&s->hist_host, bytes, hipHostMallocDefault));
    s->hist_cap = bytes;
  }
  int trips = 0;   // ceil(log2(nbins + 1)): the first power of two that is >= the number of edges
  while ((1 << trips) < nbins + 1) ++trips;
  int head_odd, segs, seg_len;
  unsigned wgs;
  const double* fu = slab_fields(s, buf, &head_odd);
  plane_work_cut(s, &segs, &seg_len, &wgs);
  HIPCHK(hipMemcpyAsync(s->formula_prog_dev, s->formula_prog_host, blob, hipMemcpyHostToDevice, s->stream));
  // no state carries over between calls: every accumulator word is zeroed on the stream first
  HIPCHK(hipMemsetAsync(s->hist_dev, 0, bytes, s->stream));
  if (s->hist_timing) HIPCHK(hipEventRecord(s->ev_hist[0], s->stream));
  hist_kernel<<<wgs, PFT_DBLOCK, 0, s->stream>>>(fu, fu + s->fs, fu + 2 * s->fs, (int)plane, head_odd, s->d.n1, n3, segs,
                                                 seg_len, P, mask_prog ? 1 : 0, (const double*)edges_dev, nbins, trips,
                                                 s->hist_dev);
  HIPCHK(hipGetLastError());
  hist_total_kernel<<<(row + 63) / 64, 256, 0, s->stream>>>(s->hist_dev, n3, row);
  HIPCHK(hipGetLastError());
  if (s->hist_timing) HIPCHK(hipEventRecord(s->ev_hist[1], s->stream));
  const bool planes = plane_heads || plane_counts;
  const size_t back = planes ? bytes : sizeof(unsigned long long) * (size_t)row;
  HIPCHK(hipMemcpyAsync(s->hist_host, s->hist_dev, back, hipMemcpyDeviceToHost, s->stream));
  const int rc = slab_wait(s, nullptr, "pft_slab_hist");
  if (rc) return rc;
  hist_record(s->hist_host, n, nbins, head, counts);
  if (planes)
    for (int k = 0; k < n3; ++k)
      hist_record(s->hist_host + (size_t)(k + 1) * row, plane, nbins, plane_heads ? &plane_heads[k] : nullptr,
                  plane_counts ? plane_counts + (size_t)k * nbins : nullptr);
  return 0;
}

int pft_slab_hist_timing(pft_slab* s, int on) { return slab_timing_set(s, &pft_slab::hist_timing, &pft_slab::ev_hist, on); }

int pft_slab_hist_last_ms(pft_slab* s, double* ms) { return slab_timing_ms(s, &pft_slab::hist_timing, &pft_slab::ev_hist, ms); }

}  // extern "C"

// ------------------------------------------------------------------------------------------
// f15: 2-D maps of formula values (pft_map.h) -- hist_kernel's interpreter and its mask-then-value
// order, but what is reduced is one record per pixel of the two axes that are kept: the value's
// counts, extrema and first / last non-zero index along the reduced axis.
//
// A pixel's accumulator is MP_WORDS 64-bit words, all zero when neutral: counts add; the minimum
// and the maximum are the complemented key and the key of diag_key under an integer max; `first`
// is kept as axis length - index and `last` as index + 1, both under an integer max (0: none).
// So partial records combine in any order to the same bits, and one hipMemsetAsync resets the map.
//
// Axes 0 and 1 (z, y: the reduced axis is strided).  A lane owns the two neighbouring pixels e, e + 1
// of the kept contiguous extent (axis 0: the whole plane; axis 1: one row of plane o) and marches
// its share of the reduced axis with both pixels' accumulators in registers (counts and indices in
// 32 bits: a line has fewer than 2^31 cells), then issues the non-zero words to the pixels' records
// with 64-bit integer atomics.  The 256 threads are laid out as pw pixel pairs x 256 / pw sub-chunks
// of the reduced axis (pw a power of two: a 50-cell row takes 32 x 8, not 25 of 256 threads), and
// map_work_cut cuts the work into items -- (plane or row) x a segment of pw pairs x a chunk of the
// reduced axis -- so that a small plane still fills the card.  A pair is read with one 16-byte load
// per field where it is 16-byte aligned at every step of the march (the run starts on a 16-byte
// boundary and the stride is even) and both pixels exist; else each element alone under its own
// test.  The two pixels of a pair and the two programs take turns through one copy of the
// interpreter, as in hist_iter.
//
// Axis 2 (x, the contiguous axis): formula_kernel's traversal -- items are segments of one plane,
// a wave takes 512 consecutive elements per iteration with coalesced 16-byte loads -- and a wave's
// window spans a few rows.  The wave keeps the partial record of its current row: the counts in
// scalar registers (ballot and popcount over the lanes of that row), the keys and first / last per
// lane; for each row a load's 128 elements touch (a wave-uniform loop, as diag_iter's over planes)
// the lanes of that row add theirs, and when the row changes the per-lane words are reduced by a
// shuffle maximum and lane 0 adds the row's non-zero words to the pixel's record.  While the row
// does not change nothing leaves the registers.
//
// LDS: the 30 720 bytes of the stack column.  No floating-point atomic, no compare-and-swap.
enum { MP_SELECTED = 0, MP_NONZERO, MP_NONFINITE, MP_MIN, MP_MAX, MP_FIRST, MP_LAST, MP_WORDS };
#define PFT_MAP_MIN_STEPS 16   // a thread's share of the reduced axis is not cut below this (axes 0, 1)
static_assert(sizeof(pft_map_px) == 8 * MP_WORDS, "pft_map_px is seven 64-bit words, no padding");

struct MapAcc {
  unsigned sel, nz, nf, first, last;   // (first: axis length - index, last: index + 1; 0: none)
  unsigned long long kmin, kmax;       // (0: no value yet)
};

__device__ __forceinline__ void map_acc_zero(MapAcc& a)
{
  a.sel = a.nz = a.nf = a.first = a.last = 0;
  a.kmin = a.kmax = 0;
}

// one cell into a lane's accumulator: sel -- the cell exists and is selected, x its value, `at` its
// index along the reduced axis of `len` cells
__device__ __forceinline__ void map_acc_take(MapAcc& a, bool sel, double x, unsigned at, unsigned len)
{
  const bool nz = sel && x != 0;   // (a NaN is "true")
  a.sel += sel ? 1u : 0u;
  a.nz += nz ? 1u : 0u;
  a.nf += sel && !diag_finite(x) ? 1u : 0u;
  const unsigned f = nz ? len - at : 0u, l = nz ? at + 1u : 0u;
  a.first = f > a.first ? f : a.first;
  a.last = l > a.last ? l : a.last;
  if (sel && x == x) {
    const unsigned long long key = diag_key(x);
    a.kmax = key > a.kmax ? key : a.kmax;
    a.kmin = ~key > a.kmin ? ~key : a.kmin;
  }
}

// the non-zero words of an accumulator to a pixel's record
__device__ __forceinline__ void map_acc_issue(const MapAcc& a, unsigned long long* __restrict__ dst)
{
  if (a.sel) atomicAdd(&dst[MP_SELECTED], (unsigned long long)a.sel);
  if (a.nz) atomicAdd(&dst[MP_NONZERO], (unsigned long long)a.nz);
  if (a.nf) atomicAdd(&dst[MP_NONFINITE], (unsigned long long)a.nf);
  if (a.kmin) atomicMax(&dst[MP_MIN], a.kmin);
  if (a.kmax) atomicMax(&dst[MP_MAX], a.kmax);
  if (a.first) atomicMax(&dst[MP_FIRST], (unsigned long long)a.first);
  if (a.last) atomicMax(&dst[MP_LAST], (unsigned long long)a.last);
}

// a cell's mask (entries m0..m1; m0 == m1: none) and then its value (c0..c1) on the lane's stack
// column; sel: in, the cell exists; out, it is also selected
__device__ __forceinline__ double map_cell(const FormulaProgs& P, int c0, int c1, int m0, int m1, double u, double p,
                                           double g, int i, int j, int k, double* stack, bool& sel)
{
  double x = 0.0;
#pragma unroll 1
  for (int pass = m1 > m0 ? 0 : 1; pass < 2; ++pass) {
    const double val = formula_eval(P, pass ? c0 : m0, pass ? c1 : m1, u, p, g, i, j, k, stack);
    if (pass == 0)
      sel = sel && val != 0;   // (a NaN is "true")
    else
      x = val;
  }
  return x;
}

// the cut of axes 0 and 1 (map_work_cut): 2^pw_log2 pixel pairs per workgroup, segs segments of them
// per kept extent, chunks chunks of chunk_len cells of the reduced axis
struct MapCut {
  int pw_log2, segs, chunks, chunk_len;
};

// axis 2's wave state: the partial record of row `row` of the item's plane (-1: none yet)
struct MapRow {
  int row;
  unsigned sel, nz, nf;                // wave-uniform counts
  unsigned first, last;                // per lane
  unsigned long long kmin, kmax;       // per lane
};

__device__ __forceinline__ void map_row_flush(MapRow& w, int lane, unsigned long long* __restrict__ dst)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long o;
    unsigned q;
    o = __shfl_xor(w.kmin, off, 64), w.kmin = o > w.kmin ? o : w.kmin;
    o = __shfl_xor(w.kmax, off, 64), w.kmax = o > w.kmax ? o : w.kmax;
    q = __shfl_xor(w.first, off, 64), w.first = q > w.first ? q : w.first;
    q = __shfl_xor(w.last, off, 64), w.last = q > w.last ? q : w.last;
  }
  if (lane == 0) {
    MapAcc a;
    a.sel = w.sel, a.nz = w.nz, a.nf = w.nf, a.first = w.first, a.last = w.last, a.kmin = w.kmin, a.kmax = w.kmax;
    map_acc_issue(a, dst);
  }
  w.sel = w.nz = w.nf = w.first = w.last = 0;
  w.kmin = w.kmax = 0;
}

// the lanes of row w.row add their cell (in: it exists, is selected and lies in that row)
__device__ __forceinline__ void map_row_take(MapRow& w, bool in, double x, int i, int n1)
{
  const bool nz = in && x != 0;
  w.sel += (unsigned)__popcll(__ballot(in));
  w.nz += (unsigned)__popcll(__ballot(nz));
  w.nf += (unsigned)__popcll(__ballot(in && !diag_finite(x)));
  const unsigned f = nz ? (unsigned)(n1 - i) : 0u, l = nz ? (unsigned)(i + 1) : 0u;
  w.first = f > w.first ? f : w.first;
  w.last = l > w.last ? l : w.last;
  if (in && x == x) {
    const unsigned long long key = diag_key(x);
    w.kmax = key > w.kmax ? key : w.kmax;
    w.kmin = ~key > w.kmin ? ~key : w.kmin;
  }
}

// acc: MP_WORDS words per pixel, row-major [n2][n1] (AXIS 0), [n3][n1] (1), [n3][n2] (2).
// AXIS 2: segs / seg_len are plane_work_cut's and cut is not used
template <int AXIS>
__global__ __launch_bounds__(PFT_DBLOCK) void map_kernel(const double* __restrict__ fu, const double* __restrict__ fp,
                                                         const double* __restrict__ fg, int plane, int head, int n1,
                                                         int n2, int n3, MapCut cut, int segs, int seg_len,
                                                         FormulaProgs P, int has_mask,
                                                         unsigned long long* __restrict__ acc)
{
  __shared__ double s_stack[PFT_FORMULA_SLOTS * PFT_DBLOCK];
  const int c0 = P.meta[0], c1 = P.meta[1];
  const int m0 = has_mask ? P.meta[3] : 0, m1 = has_mask ? P.meta[4] : 0;
  const int need = P.meta[2] | (has_mask ? P.meta[5] : 0);
  double* stack = s_stack + threadIdx.x;
  if (AXIS < 2) {
    const int ext = AXIS == 0 ? plane : n1;      // the kept contiguous extent
    const int len = AXIS == 0 ? n3 : n2;         // the reduced axis
    const long stride = AXIS == 0 ? plane : n1;
    const long outer = AXIS == 0 ? 1 : n3;
    const int pw = 1 << cut.pw_log2, sc = PFT_DBLOCK >> cut.pw_log2;
    const int tp = (int)threadIdx.x & (pw - 1), sub = (int)threadIdx.x >> cut.pw_log2;
    const int sub_len = (cut.chunk_len + sc - 1) / sc;
    const bool aligned = head == 0 && (stride & 1) == 0;
    const long items = outer * cut.segs * cut.chunks;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
      const int c = (int)(item % cut.chunks);
      const long t = item / cut.chunks;
      const int sg = (int)(t % cut.segs), o = (int)(t / cut.segs);
      const int e = 2 * (sg * pw + tp);
      const bool v0 = e < ext, v1 = e + 1 < ext;
      const int c_end = (c + 1) * cut.chunk_len < len ? (c + 1) * cut.chunk_len : len;
      const int r_begin = c * cut.chunk_len + sub * sub_len;
      int r_end = r_begin + sub_len < c_end ? r_begin + sub_len : c_end;
      if (!v0) r_end = r_begin;   // (no pixel: no step)
      // the two pixels' table indices along the kept axes
      int i0 = 0, j0 = 0, i1 = 0, j1 = 0;
      if (AXIS == 0) {
        if (need & FM_NEED_IJ) {
          const int e0 = v0 ? e : 0, e1 = v1 ? e + 1 : 0;
          j0 = e0 / n1, i0 = e0 - j0 * n1;
          j1 = e1 / n1, i1 = e1 - j1 * n1;
        }
      } else {
        i0 = v0 ? e : 0, i1 = v1 ? e + 1 : 0;
      }
      MapAcc a0, a1;
      map_acc_zero(a0);
      map_acc_zero(a1);
      long at = (long)o * plane + (long)r_begin * stride + e;
      for (int r = r_begin; r < r_end; ++r, at += stride) {
        double u[2] = {0.0, 0.0}, p[2] = {0.0, 0.0}, g[2] = {0.0, 0.0};
        if (aligned && v1) {
          if (need & FM_NEED_U) {
            const double2 q = *reinterpret_cast<const double2*>(fu + at);
            u[0] = q.x, u[1] = q.y;
          }
          if (need & FM_NEED_P) {
            const double2 q = *reinterpret_cast<const double2*>(fp + at);
            p[0] = q.x, p[1] = q.y;
          }
          if (need & FM_NEED_GL) {
            const double2 q = *reinterpret_cast<const double2*>(fg + at);
            g[0] = q.x, g[1] = q.y;
          }
        } else {
          if (need & FM_NEED_U) u[0] = fu[at];
          if (need & FM_NEED_P) p[0] = fp[at];
          if (need & FM_NEED_GL) g[0] = fg[at];
          if (v1 && (need & FM_NEED_U)) u[1] = fu[at + 1];
          if (v1 && (need & FM_NEED_P)) p[1] = fp[at + 1];
          if (v1 && (need & FM_NEED_GL)) g[1] = fg[at + 1];
        }
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
          bool sel = h ? v1 : true;
          const int ti = h ? i1 : i0, tj = AXIS == 0 ? (h ? j1 : j0) : r, tk = AXIS == 0 ? r : o;
          const double x = map_cell(P, c0, c1, m0, m1, h ? u[1] : u[0], h ? p[1] : p[0], h ? g[1] : g[0], ti, tj, tk,
                                    stack, sel);
          if (h == 0)
            map_acc_take(a0, sel, x, (unsigned)r, (unsigned)len);
          else
            map_acc_take(a1, sel, x, (unsigned)r, (unsigned)len);
        }
      }
      if (v0) {
        unsigned long long* dst = acc + ((size_t)o * n1 + (size_t)e) * MP_WORDS;   // (AXIS 0: o = 0)
        map_acc_issue(a0, dst);
        map_acc_issue(a1, dst + MP_WORDS);   // (all zero without a second pixel: nothing is issued)
      }
    }
  } else {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    MapRow w;
    w.row = -1;
    w.sel = w.nz = w.nf = w.first = w.last = 0;
    w.kmin = w.kmax = 0;
    const long items = (long)n3 * segs;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
      const ItemFrame it = item_frame(item, segs, seg_len, plane, head);
      const int k = it.k, first = it.first, r_lo = it.r_lo, r_hi = it.r_hi, span = it.span;
      const double* wu = fu + it.e_base;   // (e_base = -1: one before the run, never read at r = 0)
      const double* wp = fp + it.e_base;
      const double* wg = fg + it.e_base;
      unsigned long long* rows = acc + (size_t)k * n2 * MP_WORDS;
      for (int r0 = PFT_DIAG_WAVE_ELEMS * wave; r0 < span; r0 += PFT_DIAG_WAVE_ELEMS * (PFT_DBLOCK / 64)) {
        const bool full = r0 >= r_lo && r0 + PFT_DIAG_WAVE_ELEMS <= r_hi;
#pragma unroll 1
        for (int jj = 0; jj < PFT_DIAG_UNROLL; ++jj) {
          const int rb = r0 + 128 * jj, r = rb + 2 * lane;
          // the load's existing elements [wa, wb] (wave-uniform)
          const int wa = rb > r_lo ? rb : r_lo, wb = (rb + 128 < r_hi ? rb + 128 : r_hi) - 1;
          if (wb < wa) continue;
          double u[2] = {0.0, 0.0}, p[2] = {0.0, 0.0}, g[2] = {0.0, 0.0};
          bool v[2];
          formula_load(full, need, wu, wp, wg, r, r_lo, r_hi, u, p, g, v);
          double x0 = 0.0, x1 = 0.0;
          bool s0 = false, s1 = false;
          int i0 = 0, j0 = 0, i1 = 0, j1 = 0;
#pragma unroll 1
          for (int h = 0; h < 2; ++h) {
            const bool vh = h ? v[1] : v[0];
            // the node's place in its plane; a slot outside the item evaluates node 0 (inside every
            // table) and is left out of every count below
            const int e = vh ? first + (r + h - r_lo) : 0;
            const int j = e / n1, i = e - j * n1;
            bool sel = vh;
            const double x = map_cell(P, c0, c1, m0, m1, h ? u[1] : u[0], h ? p[1] : p[0], h ? g[1] : g[0], i, j, k,
                                      stack, sel);
            if (h == 0)
              x0 = x, s0 = sel, i0 = i, j0 = j;
            else
              x1 = x, s1 = sel, i1 = i, j1 = j;
          }
          const int ja = (first + (wa - r_lo)) / n1, jb = (first + (wb - r_lo)) / n1;
          for (int jr = ja; jr <= jb; ++jr) {
            if (jr != w.row) {
              if (w.row >= 0) map_row_flush(w, lane, rows + (size_t)w.row * MP_WORDS);
              w.row = jr;
            }
            map_row_take(w, s0 && j0 == jr, x0, i0, n1);
            map_row_take(w, s1 && j1 == jr, x1, i1, n1);
          }
        }
      }
      // (the next item is another plane or another wave's rows: nothing is kept across items)
      if (w.row >= 0) map_row_flush(w, lane, rows + (size_t)w.row * MP_WORDS);
      w.row = -1;
    }
  }
}

// The cut of axes 0 and 1 into work items, beside plane_work_cut and against the same cap of 8
// workgroups per CU: the workgroup's threads are 2^pw_log2 pixel pairs (the first power of two that
// covers the kept extent's pairs, 256 at most) x the sub-chunks that are left; the reduced axis is
// cut into as many chunks as the cap allows, but a thread's share stays PFT_MAP_MIN_STEPS cells or
// more: every chunk ends with up to 7 atomics per pixel.  An item is chunk c of segment g of the
// kept extent o (axis 0: the plane, o = 0; axis 1: the row of plane o), item = (o * segs + g) *
// chunks + c.
static void map_work_cut(const pft_slab* s, int axis, MapCut* cut, unsigned* wgs)
{
  const long ext = axis == 0 ? s->plane : s->d.n1, len = axis == 0 ? s->d.n3 : s->d.n2, outer = axis == 0 ? 1 : s->d.n3;
  const long cap = s->diag_wgs > 0 ? s->diag_wgs : 8L * (s->n_cu > 0 ? s->n_cu : 256);
  const long pairs = (ext + 1) / 2;
  int lg = 0;
  while (lg < 8 && (1L << lg) < pairs) ++lg;
  const long pw = 1L << lg, sc = PFT_DBLOCK / pw;
  const long segs = (pairs + pw - 1) / pw;
  long want = cap / (segs * outer);
  if (want < 1) want = 1;
  long chunk_len = (len + want - 1) / want;
  if (chunk_len < PFT_MAP_MIN_STEPS * sc) chunk_len = PFT_MAP_MIN_STEPS * sc;
  if (chunk_len > len) chunk_len = len;
  const long chunks = (len + chunk_len - 1) / chunk_len;
  const long items = outer * segs * chunks;
  cut->pw_log2 = lg, cut->segs = (int)segs, cut->chunks = (int)chunks, cut->chunk_len = (int)chunk_len;
  *wgs = (unsigned)(items < cap ? items : cap);
}

extern "C" {

int pft_slab_map(pft_slab* s, int buf, const pft_ic_prog* value_prog, const pft_ic_prog* mask_prog, int axis,
                 pft_map_px* out_local)
{
  if (!s || !value_prog || !out_local || buf < 0 || buf >= PFT_BUF_COUNT || axis < 0 || axis > 2) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_map");
  const long plane = s->plane, n = (long)s->d.n3 * plane;
  const int n1 = s->d.n1, n2 = s->d.n2, n3 = s->d.n3;
  if (n > 0x7fffffffL || plane > PFT_MEANS_MAX_PLANE) return -2;
  const pft_ic_prog* list[2] = {value_prog, mask_prog};
  const int nprog = mask_prog ? 2 : 1;
  long entries = 0, tvals = 0;
  int rc_pack = formula_progs_check(s, nprog, list, &entries, &tvals);
  if (rc_pack) return rc_pack;
  FormulaProgs P;
  size_t blob = 0;
  if ((rc_pack = formula_progs_pack(s, nprog, list, entries, tvals, 0, nullptr, &P, nullptr, &blob))) return rc_pack;
  const size_t pixels = (size_t)(axis == 0 ? n2 : n3) * (size_t)(axis == 2 ? n2 : n1);
  const long axis_len = axis == 0 ? n3 : (axis == 1 ? n2 : n1);
  const size_t bytes = sizeof(unsigned long long) * MP_WORDS * pixels;
  if (bytes > s->map_cap) {
    if (s->map_dev) HIPCHK(hipFree(s->map_dev));
    if (s->map_host) HIPCHK(hipHostFree(s->map_host));
    s->map_dev = s->map_host = nullptr;
    s->map_cap = 0;
    HIPCHK(hipMalloc((void**)&s->map_dev, bytes));
    HIPCHK(hipHostMalloc((void**)&s->map_host, bytes, hipHostMallocDefault));
    s->map_cap = bytes;
  }
  int head, segs = 0, seg_len = 0;
  unsigned wgs;
  MapCut cut = {0, 0, 0, 0};
  const double* fu = slab_fields(s, buf, &head);
  if (axis == 2)
    plane_work_cut(s, &segs, &seg_len, &wgs);
  else
    map_work_cut(s, axis, &cut, &wgs);
  HIPCHK(hipMemcpyAsync(s->formula_prog_dev, s->formula_prog_host, blob, hipMemcpyHostToDevice, s->stream));
  // no state carries over between calls: every accumulator word is zeroed on the stream first
  HIPCHK(hipMemsetAsync(s->map_dev, 0, bytes, s->stream));
  if (s->map_timing) HIPCHK(hipEventRecord(s->ev_map[0], s->stream));
  const double *fp = fu + s->fs, *fg = fu + 2 * s->fs;
  const int has_mask = mask_prog ? 1 : 0;
  if (axis == 0)
    map_kernel<0><<<wgs, PFT_DBLOCK, 0, s->stream>>>(fu, fp, fg, (int)plane, head, n1, n2, n3, cut, segs, seg_len, P, has_mask,
                                                     s->map_dev);
  else if (axis == 1)
    map_kernel<1><<<wgs, PFT_DBLOCK, 0, s->stream>>>(fu, fp, fg, (int)plane, head, n1, n2, n3, cut, segs, seg_len, P, has_mask,
                                                     s->map_dev);
  else
    map_kernel<2><<<wgs, PFT_DBLOCK, 0, s->stream>>>(fu, fp, fg, (int)plane, head, n1, n2, n3, cut, segs, seg_len, P, has_mask,
                                                     s->map_dev);
  HIPCHK(hipGetLastError());
  if (s->map_timing) HIPCHK(hipEventRecord(s->ev_map[1], s->stream));
  HIPCHK(hipMemcpyAsync(s->map_host, s->map_dev, bytes, hipMemcpyDeviceToHost, s->stream));
  const int rc = slab_wait(s, nullptr, "pft_slab_map");
  if (rc) return rc;
  const double inf = __builtin_inf();
  for (size_t q = 0; q < pixels; ++q) {
    const unsigned long long* h = s->map_host + q * MP_WORDS;
    pft_map_px* o = &out_local[q];
    o->selected = (long long)h[MP_SELECTED];
    o->nonzero = (long long)h[MP_NONZERO];
    o->nonfinite = (long long)h[MP_NONFINITE];
    o->min = h[MP_MIN] ? diag_unkey(~h[MP_MIN]) : inf;
    o->max = h[MP_MAX] ? diag_unkey(h[MP_MAX]) : -inf;
    o->first = h[MP_FIRST] ? axis_len - (long long)h[MP_FIRST] : -1;
    o->last = h[MP_LAST] ? (long long)h[MP_LAST] - 1 : -1;
  }
  return 0;
}

int pft_slab_map_timing(pft_slab* s, int on) { return slab_timing_set(s, &pft_slab::map_timing, &pft_slab::ev_map, on); }

int pft_slab_map_last_ms(pft_slab* s, double* ms) { return slab_timing_ms(s, &pft_slab::map_timing, &pft_slab::ev_map, ms); }

}  // extern "C"
