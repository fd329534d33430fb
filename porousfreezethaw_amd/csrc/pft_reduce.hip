// pft_reduce.hip -- reductions over the resident state: the ice diagnostics (diag_kernel, f5) and
// the exact means and z-profiles (means_kernel, f6), with their host API.
#include "pft_slab.h"

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

extern "C" {

int pft_slab_diag(pft_slab* s, int buf, const pft_diag_opts* opts, pft_diag* out, long long* ice_per_plane)
{
  if (!s || !out || buf < 0 || buf >= PFT_BUF_COUNT) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_diag");
  const long plane = s->plane, n = (long)s->d.n3 * plane;
  const size_t bytes = sizeof(unsigned long long) * (size_t)(PFT_DIAG_HEAD + s->d.n3);
  if (!s->diag_dev) HIPCHK(hipMalloc((void**)&s->diag_dev, bytes));
  if (!s->diag_host) HIPCHK(hipHostMalloc((void**)&s->diag_host, bytes, hipHostMallocDefault));
  // interior planes 1..n3 of each field; the ghost planes 0, n3+1 and the far planes are never read
  const double* fu = s->buf[buf] + plane;
  const int head = (int)(((uintptr_t)fu >> 3) & 1);   // (the field stride is even: the same for u, p, gl)
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

int pft_slab_diag_timing(pft_slab* s, int on)
{
  if (!s) return -2;
  for (int i = 0; i < 2 && on; ++i)
    if (!s->ev_diag[i]) HIPCHK(hipEventCreate(&s->ev_diag[i]));
  s->diag_timing = on ? 1 : 0;
  return 0;
}

int pft_slab_diag_last_ms(pft_slab* s, double* ms)
{
  if (!s || !ms || !s->diag_timing) return -2;
  float f = 0.0f;
  HIPCHK(hipEventElapsedTime(&f, s->ev_diag[0], s->ev_diag[1]));
  *ms = f;
  return 0;
}

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
__device__ __forceinline__ void means_flush(MeansPair& st, int lane, unsigned long long* s_all, unsigned long long* s_msk)
{
  const long long a0 = means_wave_sum(st.a0), a1 = means_wave_sum(st.a1), a2 = means_wave_sum(st.a2);
  const long long m0 = means_wave_sum(st.m0), m1 = means_wave_sum(st.m1), m2 = means_wave_sum(st.m2);
  if (lane == 0) {
    if (a0) atomicAdd(&s_all[st.cur], (unsigned long long)a0);
    if (a1) atomicAdd(&s_all[st.cur + 1], (unsigned long long)a1);
    if (a2) atomicAdd(&s_all[st.cur + 2], (unsigned long long)a2);
    if (m0) atomicAdd(&s_msk[st.cur], (unsigned long long)m0);
    if (m1) atomicAdd(&s_msk[st.cur + 1], (unsigned long long)m1);
    if (m2) atomicAdd(&s_msk[st.cur + 2], (unsigned long long)m2);
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
// into st; n_all / n_msk: the wave-uniform counts of the cells that entered
template <int NE, int I0, int I1>
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
    n_msk += __popcll(__ballot(fin && msk[i]));
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
      st.m0 += msk[i] ? e0 : 0u, st.m1 += msk[i] ? e1 : 0u, st.m2 += msk[i] ? e2 : 0u;
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
      st.m0 += msk[i] ? d0 : 0, st.m1 += msk[i] ? d1 : 0, st.m2 += msk[i] ? d2 : 0;
    }
    return;
  }
#pragma unroll
  for (int i = I0; i < I1; ++i) {
    const unsigned long long m_act = __ballot(act[i]);
    if (!m_act) continue;
    if (!__ballot(act[i] && c[i] == st.cur)) {
      means_flush(st, lane, s_all, s_msk);
      st.cur = __builtin_amdgcn_readfirstlane(__shfl(c[i], (int)__ffsll((long long)m_act) - 1, 64));
    }
    long long d0, d1, d2;
    means_signed_digits(x[i], act[i], d0, d1, d2);
    const bool here = c[i] == st.cur;            // (inactive lanes: zero digits, either way nothing)
    st.a0 += here ? d0 : 0, st.a1 += here ? d1 : 0, st.a2 += here ? d2 : 0;
    st.m0 += here && msk[i] ? d0 : 0, st.m1 += here && msk[i] ? d1 : 0, st.m2 += here && msk[i] ? d2 : 0;
    if (act[i] && !here) {
      if (d0) atomicAdd(&s_all[c[i]], (unsigned long long)d0);
      if (d1) atomicAdd(&s_all[c[i] + 1], (unsigned long long)d1);
      if (d2) atomicAdd(&s_all[c[i] + 2], (unsigned long long)d2);
      if (msk[i]) {
        if (d0) atomicAdd(&s_msk[c[i]], (unsigned long long)d0);
        if (d1) atomicAdd(&s_msk[c[i] + 1], (unsigned long long)d1);
        if (d2) atomicAdd(&s_msk[c[i] + 2], (unsigned long long)d2);
      }
    }
  }
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
    const int k = (int)(item / segs), j = (int)(item - (long)k * segs);
    const int first = j * seg_len;                                    // within the plane
    const int len = plane - first < seg_len ? plane - first : seg_len;
    const long a = (long)k * plane + first;                           // within the run of n3 planes
    // the frame: elements r = 0 .. span - 1 stand for e_base + r of the run, e_base on a 16-byte
    // boundary at or one below a; of them [r_lo, r_hi) are the item's (nothing else is read)
    const long e_base = 2 * ((a + head) >> 1) - head;
    const int r_lo = (int)(a - e_base), r_hi = r_lo + len;
    const int span = (r_hi + 1) & ~1;
    const double* wu = fu + e_base;   // (e_base = -1: one before the run, never read at r = 0)
    const double* wp = fp + e_base;
    const double* wg = fg + e_base;
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
  // interior planes 1..n3 of each field; the ghost planes 0, n3+1 and the far planes are never read
  const double* fu = s->buf[buf] + plane;
  const int head = (int)(((uintptr_t)fu >> 3) & 1);   // (the field stride is even: the same for u, p, gl)
  // at most `cap` workgroups (8 per CU), each inside one plane: a plane is cut into as many
  // segments as the cap allows, each a whole number of workgroup iterations; with fewer workgroups
  // than planes a workgroup takes several planes in turn
  const long cap = s->diag_wgs > 0 ? s->diag_wgs : 8L * (s->n_cu > 0 ? s->n_cu : 256);
  const long wg_elems = 2L * PFT_DIAG_WG_PAIRS;
  long want = cap / s->d.n3;
  if (want < 1) want = 1;
  const long seg_len = ((plane + want - 1) / want + wg_elems - 1) / wg_elems * wg_elems;
  const long segs = (plane + seg_len - 1) / seg_len;
  const long items = segs * s->d.n3;
  const long wgs = items < cap ? items : cap;
  const double p_thr = opts ? opts->p_thr : 0.5, gl_thr = opts ? opts->gl_thr : 0.5;
  // no state carries over between calls: every accumulator word is zeroed on the stream first
  HIPCHK(hipMemsetAsync(s->means_dev, 0, bytes, s->stream));
  if (s->means_timing) HIPCHK(hipEventRecord(s->ev_means[0], s->stream));
  means_kernel<<<(unsigned)wgs, PFT_DBLOCK, 0, s->stream>>>(fu, fu + s->fs, fu + 2 * s->fs, (int)plane, head, s->d.n3,
                                                            (int)segs, (int)seg_len, p_thr, gl_thr, s->means_dev);
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

int pft_slab_means_timing(pft_slab* s, int on)
{
  if (!s) return -2;
  for (int i = 0; i < 2 && on; ++i)
    if (!s->ev_means[i]) HIPCHK(hipEventCreate(&s->ev_means[i]));
  s->means_timing = on ? 1 : 0;
  return 0;
}

int pft_slab_means_last_ms(pft_slab* s, double* ms)
{
  if (!s || !ms || !s->means_timing) return -2;
  float f = 0.0f;
  HIPCHK(hipEventElapsedTime(&f, s->ev_means[0], s->ev_means[1]));
  *ms = f;
  return 0;
}

}  // extern "C"
