// pft_kernels.hip -- the hand-written step kernels for gfx950 (MI355X), the slab object's API and
// the pft_hip_* C-ABI shim.
//
// The hot path of RK_MPI_SA_solve (RK_MPI_SAsolver_hybrid2.c:351-766) with the intertrack
// right-hand side (equation.c:566-884) fused per Merson stage: each stage is ONE kernel that
// evaluates the 7-point RHS at a cell and immediately applies that stage's pointwise combine
// (hybrid2.c:378-450), the error norm (:507-524) and the candidate update (:657-668).  Every
// floating-point operation is the reference's, in the reference's order, with contraction
// disabled (-ffp-contract=off and the pragma below), so results are bit-identical to the CPU
// reference for every calc_mode (mode 2's cosh is the C library's algorithm restated, pft_cosh.h:
// x86-64 glibc 2.28 and later with its FMA build of exp, which produced the golden vectors).
//
// Memory: per slab, a field is (n3+2) planes of n1*n2 doubles (one ghost plane each side, filled
// only at slab interfaces) between two far ghost planes (the pair kernels' two-plane halo).  Mirror / Dirichlet walls (equation.c:113-263) are folded into the
// neighbour selection: the first mirrored ghost equals the boundary cell itself.
//
// Launch geometry: a 256-thread workgroup owns 256 consecutive (i,j) columns of the flattened
// plane (fully coalesced 2 KiB loads) and marches `kz` planes in z with the z-neighbours of all
// three fields in registers (2.5-D blocking).  x/y neighbours come from the L1/L2; the linear
// workgroup id is remapped so that the 8 XCDs each take a contiguous run of tiles (their y
// neighbours then share the XCD's L2, cdna_hip_programming.md T1).
//
// The halo exchange (pft_halo.hip), the device IC (pft_ic.hip), the reductions (pft_reduce.hip) and
// the snapshots (pft_snap.hip) are translation units of their own over pft_slab.h, which holds the
// slab object and what the files share.
#include "pft_slab.h"
#include "pft_zplan.h"
static_assert(PFT_K_BOUNDARY == PFT_ZP_BOUNDARY && PFT_K_BOUNDARY2 == PFT_ZP_BOUNDARY2 && PFT_K_INLINE == PFT_ZP_INLINE &&
              PFT_K_ENDS_FIRST == PFT_ZP_ENDS_FIRST, "pft_zplan.h restates the range codes of pft_hip.h");

#include "pft_cosh.h"

#pragma clang fp contract(off)

__thread char g_err[256];

int fail(hipError_t e, const char* what)
{
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  // the failed call also left e as the thread's "last error": reset it, or the next launch's
  // hipGetLastError() check would report it again (e.g. after an allocation that found the HBM full)
  (void)hipGetLastError();
  return -(int)e - 1000;
}

// ------------------------------------------------------------------------------------------
// model arithmetic (equation.c:330-421, 650-731, 835-874), operation order preserved

struct Col {           // one field at a cell: centre and its 6 face neighbours
  double c, xm, xp, ym, yp, zm, zp;
};

__device__ __forceinline__ double lam_of(const pft_consts& c, double p, double g)
{
  return g * c.lam_g + (1.0 - g) * (p * c.lam_i + (1.0 - p) * c.lam_w);
}

__device__ __forceinline__ double sshape(const pft_consts& c, double x)
{
  if (x <= c.p_eps0) return 0.0;
  if (x >= c.p_eps1) return 1.0;
  x -= c.p_eps0;
  return x * x * (c.e23 - c.e32 * x);
}

// n / c.alpha, bit for bit the compiler's IEEE division, which on gfx950 is
//   d0 = div_scale(alpha; alpha, n)   d1 = div_scale(n; alpha, n)   (powers of two keeping 1/d0 and
//   r = rcp(d0), two Newton steps: e = fma(-d0, r, 1), r = fma(r, e, r)       the quotient normal)
//   q = d1 * r;  e = fma(-d0, q, d1);  div_fixup(div_fmas(e, r, q), alpha, n)
// The second line depends on alpha alone, a launch constant, and costs a transcendental and four
// FMAs at every cell.  Here r comes from c.ralpha: the same refinement, computed once on the device
// when the constants are set (div_alpha_consts_kernel) and stored times the power of two that
// brings it to (1, 2].  d0 is alpha times a power of two, and the refinement scales with its
// operand exactly (every intermediate is normal), so r(d0) = ralpha 2^-frexp_exp(d0); where
// div_scale leaves alpha as it is, that is the very r the compiler's sequence has.  No branch and
// no range check: scaling and special cases stay with div_scale and div_fixup as before.
// -DPFT_DIV_ALPHA_HOIST=0: the plain `/` (A/B).
#ifndef PFT_DIV_ALPHA_HOIST
#define PFT_DIV_ALPHA_HOIST 1
#endif
__device__ __forceinline__ double div_alpha(double n, const pft_consts& c)
{
#if PFT_DIV_ALPHA_HOIST && defined(__HIP_DEVICE_COMPILE__)
  bool sd, sn;
  const double d0 = __builtin_amdgcn_div_scale(n, c.alpha, false, &sd);
  const double d1 = __builtin_amdgcn_div_scale(n, c.alpha, true, &sn);
  const double r = __builtin_ldexp(c.ralpha, -__builtin_amdgcn_frexp_exp(d0));
  const double q = d1 * r;
  const double e = __builtin_fma(-d0, q, d1);
  return __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(e, r, q, sn), c.alpha, n);
#else
  return n / c.alpha;
#endif
}

// c.ralpha for one alpha, by one lane.  Where alpha and its reciprocal are normal with room to
// spare, the refinement runs on alpha itself -- the compiler's operands for a numerator that makes
// div_scale leave alpha alone -- and the result is moved to (1, 2] (exact: a power of two).  Any
// other alpha (subnormal, huge) is first brought to [0.5, 1).
__global__ void div_alpha_consts_kernel(double alpha, double* out)
{
  const int ex = __builtin_amdgcn_frexp_exp(alpha);
  const bool plain = ex > -900 && ex < 900;
  const double d = plain ? alpha : __builtin_ldexp(alpha, -ex);
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  out[0] = plain ? __builtin_ldexp(r, ex) : r;
}

// test entry (pft_div_alpha_check): div_alpha against `/` on nh hashed bit patterns (splitmix64 of
// the index: every exponent, both signs) and on the nl patterns of list; counts the mismatches
__global__ __launch_bounds__(256) void div_alpha_check_kernel(pft_consts c, unsigned long long nh,
                                                              const unsigned long long* list, unsigned long long nl,
                                                              unsigned long long* bad)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nh + nl) return;
  unsigned long long b;
  if (i < nh) {
    b = i + 0x9E3779B97F4A7C15ULL;
    b = (b ^ (b >> 30)) * 0xBF58476D1CE4E5B9ULL;
    b = (b ^ (b >> 27)) * 0x94D049BB133111EBULL;
    b ^= b >> 31;
  } else {
    b = list[i - nh];
  }
  const double n = __longlong_as_double((long long)b);
  const double got = div_alpha(n, c), ref = n / c.alpha;
  if (__double_as_longlong(got) != __double_as_longlong(ref)) atomicAdd(bad, 1ULL);
}

// test entry (pft_cosh_eval): y[i] = pft_cosh(x[i]), mode 2's cosh on its own
__global__ __launch_bounds__(256) void cosh_eval_kernel(const double* __restrict__ x, double* __restrict__ y,
                                                        unsigned long long n)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = pft_cosh(x[i]);
}

// K (du, dp) at one cell; dgl is identically 0 (equation.c:731,874)
template <int MODE>
__device__ __forceinline__ void rhs_cell(const pft_consts& c, const Col& u, const Col& p, const Col& g,
                                         double un, double& du, double& dp)
{
  // un = u + u_noise (equation.c:676,687); only the reaction terms see the noise
  const double pc = p.c, gc = g.c, uc = u.c;
  const double rho = gc * c.rho_g + (1.0 - gc) * (pc * c.rho_i + (1.0 - pc) * c.rho_w);
  const double cp = gc * c.cp_g + (1.0 - gc) * (pc * c.cp_i + (1.0 - pc) * c.cp_w);
  const double wi = fmax(0.0, 1.0 - c.zeta * gc);
  if (MODE == 10 || MODE == 11) {
    du = 0.0;
  }
  double flux = 0.0;
  if (MODE != 10 && MODE != 11) {
    const double lxm = lam_of(c, 0.5 * (p.xm + pc), 0.5 * (g.xm + gc));
    const double lxp = lam_of(c, 0.5 * (pc + p.xp), 0.5 * (gc + g.xp));
    const double lym = lam_of(c, 0.5 * (p.ym + pc), 0.5 * (g.ym + gc));
    const double lyp = lam_of(c, 0.5 * (pc + p.yp), 0.5 * (gc + g.yp));
    const double lzm = lam_of(c, 0.5 * (p.zm + pc), 0.5 * (g.zm + gc));
    const double lzp = lam_of(c, 0.5 * (pc + p.zp), 0.5 * (gc + g.zp));
    flux = c.h1_2 * (-lxm * (-u.xm + uc) + lxp * (-uc + u.xp)) +
           c.h2_2 * (-lym * (-u.ym + uc) + lyp * (-uc + u.yp)) +
           c.h3_2 * (-lzm * (-u.zm + uc) + lzp * (-uc + u.zp));
  }
  if (MODE == 2) {
    const double ch = pft_cosh(c.gamma * (uc - c.u_star));
    const double dpdu = (c.mhg / (ch * ch)) * wi;
    const double d = flux / (rho * (cp - c.L * dpdu));
    du = d;
    dp = dpdu * d;
  } else {
    double dpdt = c.h1_2 * (-(-p.xm + pc) + (-pc + p.xp)) +
                  c.h2_2 * (-(-p.ym + pc) + (-pc + p.yp)) +
                  c.h3_2 * (-(-p.zm + pc) + (-pc + p.zp));
    if (MODE == 0 || MODE == 10) {
      const double v1 = c.h1d2 * (-p.xm + p.xp);
      const double v2 = c.h2d2 * (-p.ym + p.yp);
      const double v3 = c.h3d2 * (-p.zm + p.zp);
      const double gn = sqrt(v1 * v1 + v2 * v2 + v3 * v3) + 1E-10;
      dpdt += c.xi2a * pc * (1.0 - pc) * (pc - 0.5) - c.bam * gn * (un - c.u_star);
    } else {
      dpdt += c.xi2a * pc * (1.0 - pc) * (pc - 0.5) -
              c.sam * sshape(c, pc) * sshape(c, 1.0 - pc) * fmax(pc * (1.0 - pc), 0.0) * (un - c.u_star);
    }
    dpdt = div_alpha(dpdt, c);
    dpdt *= wi;
    dp = dpdt;
    if (MODE == 0 || MODE == 1) du = (flux / rho + c.L * dpdt) / cp;
  }
}

// The same arithmetic with face reuse: a face shared by two cells computed by one thread is
// evaluated once.  Across the face between cells a (minus side) and b (plus side) the reference
// computes, at a: lp * (-u_a + u_b) with lp = lambda(0.5*(p_a+p_b), 0.5*(g_a+g_b)), and at b:
// (-lm) * (-u_a + u_b) with lm = lambda(0.5*(p_a+p_b), ...) -- the same operands in the same
// order, so lm == lp and (-lm)*d == -(lp*d) exactly; likewise the Laplacian difference
// (-p_a + p_b).  FaceT carries {lp*d, -p_a + p_b} from a to b.
struct FaceT {
  double prod, dp;
};

__device__ __forceinline__ FaceT face_of(const pft_consts& c, double pa, double ga, double ua, double pb, double gb,
                                         double ub, bool need_flux)
{
  FaceT f;
  f.dp = -pa + pb;
  f.prod = need_flux ? lam_of(c, 0.5 * (pa + pb), 0.5 * (ga + gb)) * (-ua + ub) : 0.0;
  return f;
}

// rhs_cell with the x-minus and z-minus faces given (fxm, fzm: the plus faces of the neighbours),
// returning this cell's x-plus and z-plus faces
template <int MODE>
__device__ __forceinline__ void rhs_cell_f(const pft_consts& c, const Col& u, const Col& p, const Col& g, double un,
                                           const FaceT& fxm, const FaceT& fzm, FaceT& fxp, FaceT& fzp, double& du,
                                           double& dp)
{
  constexpr bool FLUX = MODE != 10 && MODE != 11;
  const double pc = p.c, gc = g.c, uc = u.c;
  const double rho = gc * c.rho_g + (1.0 - gc) * (pc * c.rho_i + (1.0 - pc) * c.rho_w);
  const double cp = gc * c.cp_g + (1.0 - gc) * (pc * c.cp_i + (1.0 - pc) * c.cp_w);
  const double wi = fmax(0.0, 1.0 - c.zeta * gc);
  fxp = face_of(c, pc, gc, uc, p.xp, g.xp, u.xp, FLUX);
  fzp = face_of(c, pc, gc, uc, p.zp, g.zp, u.zp, FLUX);
  if (MODE == 10 || MODE == 11) du = 0.0;
  double flux = 0.0;
  if (FLUX) {
    const double lym = lam_of(c, 0.5 * (p.ym + pc), 0.5 * (g.ym + gc));
    const double lyp = lam_of(c, 0.5 * (pc + p.yp), 0.5 * (gc + g.yp));
    flux = c.h1_2 * (-fxm.prod + fxp.prod) +
           c.h2_2 * (-lym * (-u.ym + uc) + lyp * (-uc + u.yp)) +
           c.h3_2 * (-fzm.prod + fzp.prod);
  }
  if (MODE == 2) {
    const double ch = pft_cosh(c.gamma * (uc - c.u_star));
    const double dpdu = (c.mhg / (ch * ch)) * wi;
    const double d = flux / (rho * (cp - c.L * dpdu));
    du = d;
    dp = dpdu * d;
  } else {
    double dpdt = c.h1_2 * (-fxm.dp + fxp.dp) +
                  c.h2_2 * (-(-p.ym + pc) + (-pc + p.yp)) +
                  c.h3_2 * (-fzm.dp + fzp.dp);
    if (MODE == 0 || MODE == 10) {
      const double v1 = c.h1d2 * (-p.xm + p.xp);
      const double v2 = c.h2d2 * (-p.ym + p.yp);
      const double v3 = c.h3d2 * (-p.zm + p.zp);
      const double gn = sqrt(v1 * v1 + v2 * v2 + v3 * v3) + 1E-10;
      dpdt += c.xi2a * pc * (1.0 - pc) * (pc - 0.5) - c.bam * gn * (un - c.u_star);
    } else {
      dpdt += c.xi2a * pc * (1.0 - pc) * (pc - 0.5) -
              c.sam * sshape(c, pc) * sshape(c, 1.0 - pc) * fmax(pc * (1.0 - pc), 0.0) * (un - c.u_star);
    }
    dpdt = div_alpha(dpdt, c);
    dpdt *= wi;
    dp = dpdt;
    if (MODE == 0 || MODE == 1) du = (flux / rho + c.L * dpdt) / cp;
  }
}

// ------------------------------------------------------------------------------------------
// the fused stage kernel

struct StageArgs {
  const double* in;    // stage input state (u, p, gl)
  const double* x;     // solution x
  const double* k1;
  const double* k3;
  const double* k4;
  double* kout;        // K of this stage (stages 0, 1, 3, 4)
  double* out;         // next stage input (1..4) or candidate x(t+h) (5)
  unsigned long long* eps_bits;
  unsigned int* nonfinite;
  const double* noise; // u_noise [k][j][i] or null (u_noise_amp == 0)
  long fs;             // field stride (doubles)
  int n1, n2, n3, plane;
  int has_below, has_above;
  int k_begin, k_end, kz, ntile, nchunk;
  int kspan;           // planes a chunk processes from its start (kz, or 1 for the boundary planes)
  // inline boundary (merson_fused; pft_zplan.h): the first nbw workgroups produce the planes the
  // exchange sends and count themselves in *bdone
  int nbw, bends, c0, nint;
  unsigned long long* bdone;
  double T_top;        // Dirichlet value T_top(t_stage), equation.c:110
  double coef, h;
  double em0, em1, em2;
  // recompute path (merson_fused): the stage input is rebuilt from x and the K's
  const double* k2;    // K2 (stored only on this path; the reference aliases it with K3)
  double cin;          // coefficient of the stage-input combine: h3, h6, h8, h for stages 2..5
  int gwx, gty;        // merson_fused tile: gwx cell pairs x gty rows (fused_geometry)
  int gl_keep;         // stage 5: x(t+h) of gl is not stored, XN already holds it (pft_slab_set_gl_keep)
  // stage 5 (merson_fused): the last workgroup to finish publishes the error norm straight to
  // pinned host memory (pub[0] eps bits, pub[1] non-finite flag, both pre-set to a sentinel by
  // the host) and resets the accumulator; pub_count counts the finished workgroups
  unsigned long long* pub;
  unsigned int* pub_count;
  struct EpsShard* shards;   // stage 5: the error norm's per-shard accumulators (eps_arrive)
  // deferred publication (eps_reduce_publish): stage 5 stores its workgroups' partials to part;
  // stage 1 with npart > 0 reduces npart partials in its last workgroup and publishes them to pub
  unsigned long long* part;
  int npart;
  // Gated step (f4, small slabs, pft_slab_gate_*): this launch was enqueued before the step it
  // belongs to was decided.  gate -> 3 device words the previous speculative stage 1 wrote with
  // its decision (gate_decide): [0] a sequence number (the launch runs iff == gseq; the skip bit
  // never equals it), [1] t, [2] h of the step (bit patterns): the launch derives its scalars
  // from them with the solver's own expressions (gate_scalars).
  const unsigned long long* gate;
  unsigned long long gseq;
  // ... and the decision: the speculative stage 1's extra workgroup, once it has the error norm, decides
  // the step with the solver's own controller (pft_stepctl.h) and writes it to gdev (for the launches gated
  // on it) and to pinned gpin (for the host, which takes its own decision and compares bit for bit).  gdec_seq:
  // its number; dt, dh: t and h of the step decided (a gated launch's: from its gate); k: the solve's constants.
  unsigned long long* gdev;
  unsigned long long* gpin;
  unsigned long long gdec_seq;
  double dt, dh;
  pft_stepctl_consts k;
  int d_flip;          // test hook (env PFT_GATE_FLIP = N): every N-th accepted decision leaves the
                       // device with the last bit of its h flipped, so the host's check must discard
                       // and relaunch that step (tests/test_gate_gpu.py)
};

#define PFT_GATE_SKIP (1ULL << 63)

// a gated launch's scalars from the decided (t, h) by the function the host calls (pft_stepctl_stage; a
// gated stage 1 is the speculative one, 6) and equation.c:110 T_top: correctly rounded, the same bits
template <int STAGE>
__device__ __forceinline__ void gate_scalars(StageArgs& a, const pft_consts& c, double t, double h)
{
  const pft_stage_scalars s = pft_stepctl_stage(STAGE == 1 ? 6 : STAGE, t, h);
  a.coef = s.coef;
  a.h = h;
  a.cin = s.cin;
  a.T_top = s.ts < c.phase_switch_time ? c.top_temp1 : c.top_temp2;
  if (STAGE == 5) a.gl_keep = a.gl_keep && isfinite(a.coef);
}

// One thread: the host loops' own judgement and advance (pft_stepctl.h) of the step (t, h) whose error
// norm bits epsb / flag nf were just reduced: the next (t, h) if accepted, else a skip.  Only x^0.2 can
// differ from the host's (pft_stepctl_pow02), which keeps the gated step only if both agree bit for bit.
__device__ __forceinline__ void gate_decide(const StageArgs& a, double t, double h, unsigned long long epsb, int nf,
                                            bool have_eps)
{
  const double eps = __longlong_as_double((long long)epsb);
  unsigned long long v = a.gdec_seq | PFT_GATE_SKIP, tb = 0, hb = 0;
  if (have_eps) {
    // (no command is pending: the host enqueues nothing behind a step that ends the solve)
    const pft_step at = {t, h, 0};
    double new_h;
    const int command = pft_stepctl_judge(a.k, at, eps, nf, &new_h);
    if (pft_stepctl_accepted(command)) {
      const pft_step s = pft_stepctl_advance(a.k, at, command, new_h);
      tb = (unsigned long long)__double_as_longlong(s.t);
      hb = (unsigned long long)__double_as_longlong(s.h);
      if (a.d_flip > 0 && a.gdec_seq % (unsigned long long)a.d_flip == 0) hb ^= 1ULL;
      v = a.gdec_seq;
    }
  }
  a.gdev[1] = tb;
  a.gdev[2] = hb;
  __hip_atomic_store(a.gdev, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(a.gpin + 1, tb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(a.gpin + 2, hb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(a.gpin, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// a value the error norm never takes (a NaN pattern: the max skips NaN) nor the flag
#define PFT_PUB_SENTINEL 0xFFF8DEADBEEF0001ULL

// The error norm's max over the workgroups of a launch (hybrid2.c:507-524 over the slab), and with
// it the count of finished workgroups whose last one publishes: arrivals on one address serialise
// at the memory side (~12 ns each), so a launch of ~500 short workgroups that all finish at once
// spent ~6 us in that queue (stage 5 at 100^3: 13.5 against 7 us for stage 4).  Workgroups
// arrive on one of PFT_EPS_SHARDS shards (blockIdx % shards: the dispatcher deals consecutive
// blocks to different XCDs) and the last of each shard forwards its shard's max to the launch's
// accumulator -- the same max, a tenth of the queue.  Every word is reset by the workgroup that
// reads it last, so the next launch on the stream finds them zero.
#define PFT_EPS_SHARDS 8
struct EpsShard {
  unsigned long long max;   // bit pattern of the shard's max (non-negative doubles order as their bits)
  unsigned int nf, cnt;     // non-finite flag, finished workgroups
  unsigned long long pad[6];  // one 64-byte line per shard
};

// called by one thread per workgroup after its block-level max bm / flag bnf; pub: the pinned host
// slot of an in-kernel publication (null: the accumulator is read after the launch)
__device__ __forceinline__ void eps_arrive(double bm, int bnf, EpsShard* shards, unsigned long long* eps_bits,
                                           unsigned int* nonfinite, unsigned long long* pub, unsigned int* pub_count)
{
  const unsigned nb = gridDim.x, b = blockIdx.x % PFT_EPS_SHARDS;
  const unsigned nsh = nb < PFT_EPS_SHARDS ? nb : PFT_EPS_SHARDS;             // shards with workgroups
  const unsigned in_shard = (nb - b + PFT_EPS_SHARDS - 1) / PFT_EPS_SHARDS;   // workgroups of shard b
  EpsShard* sh = shards + b;
  if (bm > 0.0) atomicMax(&sh->max, (unsigned long long)__double_as_longlong(bm));   // NaN never wins
  if (bnf) atomicOr(&sh->nf, 1u);
  // this workgroup's atomics are performed (memory-side) before it is counted
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (atomicAdd(&sh->cnt, 1u) != in_shard - 1) return;
  const unsigned long long m = atomicExch(&sh->max, 0ULL);
  const unsigned int f = atomicExch(&sh->nf, 0u);
  atomicExch(&sh->cnt, 0u);
  if (m) atomicMax(eps_bits, m);
  if (f) atomicOr(nonfinite, 1u);
  if (!pub) return;
  // the last shard to finish reads the final max, resets the accumulator and publishes both words
  // to the host, which polls them (no publish kernel, no event: pft_slab_eps_fetch)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (atomicAdd(pub_count, 1u) != nsh - 1) return;
  const unsigned long long e = atomicExch(eps_bits, 0ULL);
  const unsigned int ff = atomicExch(nonfinite, 0u);
  atomicExch(pub_count, 0u);
  __hip_atomic_store(pub, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(pub + 1, (unsigned long long)ff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Deferred publication (single slab / ipc, the speculative path): the error-norm launch does no
// atomics at all -- each workgroup stores its (max bits, non-finite flag) to part[2 b], part[2 b + 1]
// -- and the NEXT launch on the stream, the speculative stage 1, which follows it in every step,
// reduces them in one extra workgroup and publishes to the pinned host slot while its other
// workgroups compute.  The reduction leaves the error-norm launch's critical path (its last
// workgroups spent ~1-2 us in the arrival atomics), and the kernel boundary orders the plain stores
// before the reads.  One block of 256 threads; called with the block's threads.
__device__ __forceinline__ void eps_part_load(const unsigned long long* __restrict__ part, int n, unsigned long long& m,
                                              unsigned long long& f)
{
  m = 0;
  f = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const unsigned long long b = part[2 * i], nf = part[2 * i + 1];
    m = b > m ? b : m;   // non-negative doubles (and +0) order as their bit patterns
    f |= nf;
  }
}
__device__ __forceinline__ void eps_part_publish(unsigned long long m, unsigned long long f, unsigned long long* pub,
                                                 unsigned long long* mo = nullptr, unsigned long long* fo = nullptr)
{
  __shared__ unsigned long long rm[4], rf[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long om = __shfl_xor(m, off, 64), of = __shfl_xor(f, off, 64);
    m = om > m ? om : m;
    f |= of;
  }
  if ((threadIdx.x & 63) == 0) {
    rm[threadIdx.x >> 6] = m;
    rf[threadIdx.x >> 6] = f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
      m = rm[w] > m ? rm[w] : m;
      f |= rf[w];
    }
    __hip_atomic_store(pub, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pub + 1, f ? 1ULL : 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (mo) *mo = m;
    if (fo) *fo = f;
  }
}
__device__ __forceinline__ void eps_reduce_publish(const unsigned long long* __restrict__ part, int n,
                                                   unsigned long long* pub, unsigned long long* mo = nullptr,
                                                   unsigned long long* fo = nullptr)
{
  unsigned long long m, f;
  eps_part_load(part, n, m, f);
  eps_part_publish(m, f, pub, mo, fo);
}

// a workgroup's contribution in the deferred form
__device__ __forceinline__ void eps_store_part(unsigned long long* part, double bm, int bnf)
{
  part[2 * blockIdx.x] = bm > 0.0 ? (unsigned long long)__double_as_longlong(bm) : 0ULL;   // NaN never wins
  part[2 * blockIdx.x + 1] = bnf ? 1ULL : 0ULL;
}

__global__ __launch_bounds__(256) void eps_reduce_kernel(const unsigned long long* part, int n,
                                                         unsigned long long* pub)
{
  eps_reduce_publish(part, n, pub);
}


template <int STAGE, bool GLS>
__device__ __forceinline__ double combine(const StageArgs& a, int q, long o, double K, double* m, bool& nf)
{
  // returns the value written to `out` (not used for stage 0)
  const double xv = a.x[q * a.fs + o];
  if (STAGE == 1) {
    a.kout[q * a.fs + o] = K;
    a.out[q * a.fs + o] = K * a.coef + xv;                               // hybrid2.c:388
  } else if (STAGE == 2) {
    const double k1 = a.k1[q * a.fs + o];
    a.out[q * a.fs + o] = (k1 + K) * a.coef + xv;                        // :408
  } else if (STAGE == 3) {
    const double k1 = a.k1[q * a.fs + o];
    a.kout[q * a.fs + o] = K;
    a.out[q * a.fs + o] = (k1 + 3.0 * K) * a.coef + xv;                  // :428
  } else if (STAGE == 4) {
    const double k1 = a.k1[q * a.fs + o], k3 = a.k3[q * a.fs + o];
    a.kout[q * a.fs + o] = K;
    a.out[q * a.fs + o] = (0.5 * k1 - 1.5 * k3 + 2.0 * K) * a.h + xv;   // :449
  } else if (STAGE == 5) {
    const double k1 = a.k1[q * a.fs + o], k3 = a.k3[q * a.fs + o], k4 = a.k4[q * a.fs + o];
    const double em = q == 0 ? a.em0 : (q == 1 ? a.em1 : a.em2);
    const double e = em * fabs(0.2 * k1 - 0.9 * k3 + 0.8 * k4 - 0.1 * K);   // :521
    if (e > *m) *m = e;                                                  // :522 (NaN never wins)
    nf |= !isfinite(e);
    a.out[q * a.fs + o] = xv + a.coef * (0.5 * (k1 + K) + 2.0 * k4);   // :667
  }
  return 0.0;
}

template <int STAGE, int MODE, bool GLS>
__global__ __launch_bounds__(PFT_BLOCK) void merson_stage(StageArgs a, pft_consts c)
{
  int tile, chunk, kb, ke;
  pft_zplan_chunk_flat((int)blockIdx.x, a.ntile, a.nchunk, &tile, &chunk);
  const int cell = tile * PFT_BLOCK + threadIdx.x;
  const bool active = cell < a.plane;
  const int cc = active ? cell : a.plane - 1;
  const int j = cc / a.n1, i = cc - j * a.n1;
  pft_zplan_planes(chunk, false, a.n3, a.k_begin, a.k_end, a.kz, a.kspan, &kb, &ke);

  // neighbour offsets within a plane, mirrored at the x/y walls (equation.c:137-161)
  const int oxm = i > 0 ? -1 : 0, oxp = i < a.n1 - 1 ? 1 : 0;
  const int oym = j > 0 ? -a.n1 : 0, oyp = j < a.n2 - 1 ? a.n1 : 0;

  const double* fin[3] = {a.in, a.in + a.fs, GLS ? a.x + 2 * a.fs : a.in + 2 * a.fs};

  double m = 0.0;
  bool nf = false;
  // software pipeline over the z-march (the loads of plane k+1's x/y neighbours and of plane
  // k+2's centre are in flight while plane k is computed):
  //   zm/zc/zp: centres of planes k-1, k, k+1;  nb: x/y neighbours of plane k;
  //   zn: centre of plane k+2 and nn: x/y neighbours of plane k+1 (prefetched)
  double zm[3], zc[3], zp[3], zn[3], nb[3][4], nn[3][4];
  if (kb < ke) {
    const long o0 = (long)(kb + 1) * a.plane + cc;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      zc[q] = fin[q][o0];
      // bottom wall: mirror (equation.c:164-174); slab interface: ghost plane
      zm[q] = (kb == 0 && !a.has_below) ? zc[q] : fin[q][o0 - a.plane];
      zp[q] = (kb == a.n3 - 1 && !a.has_above) ? zc[q] : fin[q][o0 + a.plane];
      nb[q][0] = fin[q][o0 + oxm];
      nb[q][1] = fin[q][o0 + oxp];
      nb[q][2] = fin[q][o0 + oym];
      nb[q][3] = fin[q][o0 + oyp];
    }
  }
  for (int k = kb; k < ke; ++k) {
    const long o = (long)(k + 1) * a.plane + cc;
    const bool top = (k == a.n3 - 1) && !a.has_above;
    // pointwise operands of this plane's stage combine, issued before the stencil arithmetic
    double xv[3], k1v[3], k3v[3], k4v[3];
    if (STAGE >= 1) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (GLS && q == 2) continue;
        xv[q] = a.x[q * a.fs + o];
        if (STAGE >= 2) k1v[q] = a.k1[q * a.fs + o];
        if (STAGE >= 4) k3v[q] = a.k3[q * a.fs + o];
        if (STAGE >= 5) k4v[q] = a.k4[q * a.fs + o];
      }
    }
    // prefetch for the next plane
    if (k + 1 < ke) {
      const long o1 = o + a.plane;
      const bool top2 = (k + 1 == a.n3 - 1) && !a.has_above;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        nn[q][0] = fin[q][o1 + oxm];
        nn[q][1] = fin[q][o1 + oxp];
        nn[q][2] = fin[q][o1 + oym];
        nn[q][3] = fin[q][o1 + oyp];
        zn[q] = top2 ? 0.0 : fin[q][o1 + a.plane];
      }
    }
    Col col[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      col[q].c = zc[q];
      col[q].xm = nb[q][0];
      col[q].xp = nb[q][1];
      col[q].ym = nb[q][2];
      col[q].yp = nb[q][3];
      col[q].zm = zm[q];
      col[q].zp = top ? zc[q] : zp[q];               // top wall: mirror ...
    }
    if (top) col[0].zp = a.T_top;                    // ... except Dirichlet u (equation.c:175-183)
    double du = 0.0, dp = 0.0;
    const double un = a.noise ? zc[0] + a.noise[(long)k * a.plane + cc] : zc[0];
    rhs_cell<MODE>(c, col[0], col[1], col[2], un, du, dp);
    if (active) {
      if (STAGE == 0) {
        a.kout[o] = du;
        a.kout[a.fs + o] = dp;
        a.kout[2 * a.fs + o] = 0.0;
      } else {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          if (GLS && q == 2) continue;
          const double K = q == 0 ? du : (q == 1 ? dp : 0.0);   // dgl = 0 (equation.c:731)
          const long e = q * a.fs + o;
          if (STAGE == 1) {
            a.kout[e] = K;
            a.out[e] = K * a.coef + xv[q];                                         // hybrid2.c:388
          } else if (STAGE == 2) {
            a.out[e] = (k1v[q] + K) * a.coef + xv[q];                              // :408
          } else if (STAGE == 3) {
            a.kout[e] = K;
            a.out[e] = (k1v[q] + 3.0 * K) * a.coef + xv[q];                        // :428
          } else if (STAGE == 4) {
            a.kout[e] = K;
            a.out[e] = (0.5 * k1v[q] - 1.5 * k3v[q] + 2.0 * K) * a.h + xv[q];     // :449
          } else if (STAGE == 5) {
            const double em = q == 0 ? a.em0 : (q == 1 ? a.em1 : a.em2);
            const double ev = em * fabs(0.2 * k1v[q] - 0.9 * k3v[q] + 0.8 * k4v[q] - 0.1 * K);  // :521
            if (ev > m) m = ev;                                                    // :522 NaN never wins
            nf |= !isfinite(ev);
            a.out[e] = xv[q] + a.coef * (0.5 * (k1v[q] + K) + 2.0 * k4v[q]);      // :667
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      zm[q] = zc[q];
      zc[q] = zp[q];
      zp[q] = zn[q];
#pragma unroll
      for (int d = 0; d < 4; ++d) nb[q][d] = nn[q][d];
    }
  }

  if (STAGE == 5) {
    // block max of the error norm (exact, order-independent), one atomic per block
    __shared__ double red[PFT_BLOCK / 64];
    __shared__ int rnf[PFT_BLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(m, off, 64);
      if (o > m) m = o;
    }
    const int anynf = __any(nf);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      red[w] = m;
      rnf[w] = anynf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double bm = red[0];
      int bnf = rnf[0];
      for (int k = 1; k < PFT_BLOCK / 64; ++k) {
        if (red[k] > bm) bm = red[k];
        bnf |= rnf[k];
      }
      // non-negative doubles order like their bit patterns
      if (bm > 0.0) atomicMax(a.eps_bits, (unsigned long long)__double_as_longlong(bm));
      if (bnf) atomicOr(a.nonfinite, 1u);
    }
  }
}

// ------------------------------------------------------------------------------------------
// the LDS-tiled fused stage kernel (n1 even): a 256-thread workgroup owns a TX x TY tile of the
// (x, y) plane, two x-adjacent cells per thread (16-byte loads and stores everywhere), and marches
// kz planes in z.  Plane k of the stage input sits in LDS with a halo (one row above/below, one
// 16-byte pair left/right), so each input value is fetched from memory once per plane instead
// of five times; plane k+1 is staged into the second LDS buffer while plane k is computed (the
// thread's own centre values double as the z+1 neighbours, the halo ring is one 16-byte load per
// thread).  The z-neighbours stay in registers.

typedef double dbl2 __attribute__((ext_vector_type(2)));

// LDS doubles per field and plane of merson_fused: (2 gwx + 4)(gty + 2) <= 680 (64 x 8 tiles)
#define PFT_FUSED_LF 680

// (non-temporal loads measured -25%, non-temporal stores +-0: plain accesses)
__device__ __forceinline__ dbl2 ld2(const double* p) { return *reinterpret_cast<const dbl2*>(p); }
__device__ __forceinline__ void st2(double* p, dbl2 v) { *reinterpret_cast<dbl2*>(p) = v; }

// ------------------------------------------------------------------------------------------
// the recompute kernel (default): an LDS tile, and no stage-input ("aux") array exists.
// The reference writes aux = combine(x, K...) after each stage and the next RHS reads it
// (hybrid2.c:378-450); here each stage kernel reads x and the K's its input is made of and
// evaluates the same combine, with the same operands in the same order, while staging the plane
// into LDS -- bit-identical inputs, and per cell-step 54 instead of 72 doubles of HBM traffic
// (SURVEY 8(d)'s "fused lower bound", 432 B).  Stage s writes only K_s (stage 5: x(t+h)).

struct Ops {             // operands of one 16-byte cell pair of one field
  dbl2 x, k1, k2, k3, k4;
};

template <int STAGE, bool GLS>
__device__ __forceinline__ void load_ops(const StageArgs& a, int q, long o, Ops& r)
{
  r.x = ld2(a.x + q * a.fs + o);
  if (GLS && q == 2) return;                     // dgl == 0: the gl input is x (F4)
  if (q == 2) {
    // gl's K's are the literal 0.0 the model's RHS writes for dgl (equation.c:731,874): never
    // stored, never loaded; the stage combines still run on them (stage_in, stage 5), so the gl
    // stage inputs and x(t+h) carry the reference's bits, signed zeros included
    constexpr dbl2 z = {0.0, 0.0};
    r.k1 = z; r.k2 = z; r.k3 = z; r.k4 = z;
    return;
  }
  if (STAGE >= 2 && STAGE != 3) r.k1 = ld2(a.k1 + q * a.fs + o);
  if (STAGE == 3) r.k2 = ld2(a.k2 + q * a.fs + o);   // S = K1 + K2, stored by stage 2
  if (STAGE >= 4) r.k3 = ld2(a.k3 + q * a.fs + o);
  if (STAGE == 5) r.k4 = ld2(a.k4 + q * a.fs + o);
}

template <int STAGE, bool GLS>
__device__ __forceinline__ dbl2 stage_in(const StageArgs& a, int q, const Ops& r)
{
  if (STAGE <= 1 || (GLS && q == 2)) return r.x;
  dbl2 v;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (STAGE == 2) v[s] = r.k1[s] * a.cin + r.x[s];                                      // hybrid2.c:388
    if (STAGE == 3) v[s] = r.k2[s] * a.cin + r.x[s];                                      // :408 (S = K1 + K2)
    if (STAGE == 4) v[s] = (r.k1[s] + 3.0 * r.k3[s]) * a.cin + r.x[s];                    // :428
    if (STAGE == 5) v[s] = (0.5 * r.k1[s] - 1.5 * r.k3[s] + 2.0 * r.k4[s]) * a.cin + r.x[s];  // :449
  }
  return v;
}

template <bool GLS>
__device__ __forceinline__ void keep5(int q, const Ops& r, dbl2& x, dbl2& k1, dbl2& k4, dbl2& E)
{
  x = r.x;
  if (q == 2) return;
  k1 = r.k1;
  k4 = r.k4;
#pragma unroll
  for (int s = 0; s < 2; ++s) E[s] = 0.2 * r.k1[s] - 0.9 * r.k3[s] + 0.8 * r.k4[s];   // hybrid2.c:521 prefix
}

template <int STAGE, int MODE, bool GLS>
__global__ __launch_bounds__(PFT_FBLOCK) __attribute__((amdgpu_waves_per_eu(STAGE >= 1 ? 2 : 3))) void merson_fused(StageArgs a, pft_consts c)
{
  // tile geometry chosen by the host per grid (fused_geometry): gwx pairs x gty rows, so that the
  // tiles fit n1 and n2 without mostly-idle edge workgroups (n1 = 200: 50 x 10 cells)
  const int WX = a.gwx, TY = a.gty, TX = 2 * WX, LW = TX + 4, LH = TY + 2, NH = LW + 2 * TY;
  __shared__ __attribute__((aligned(16))) double lds[2][3][PFT_FUSED_LF];

  // A gated launch runs iff the step it belongs to was accepted, on the decided (t, h) (gate words
  // [0] sequence, [1] t, [2] h).  The words are loaded here, beside the prologue's operand loads
  // (which need no scalar of the step), and checked after them: one memory round trip before the
  // stencil instead of two dependent ones (the check and then t, h) ahead of it.
  unsigned long long gw0 = 0, gw1 = 0, gw2 = 0;
  if (a.gate) {
    gw0 = __hip_atomic_load(a.gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    gw1 = a.gate[1];
    gw2 = a.gate[2];
  }
  if (STAGE == 1 && (a.npart > 0 || a.gdev) && (int)blockIdx.x == a.nbw + a.nint) {
    // the extra workgroup of a speculative stage 1: the previous launch's error norm, then (gated
    // steps) the decision on the step it ended
    unsigned long long m = 0, f = 0;
    if (a.npart > 0) eps_part_load(a.part, a.npart, m, f);
    if (a.gate) {
      if (gw0 != a.gseq) return;       // (uniform: every thread read the same word)
      a.dt = __longlong_as_double((long long)gw1);
      a.dh = __longlong_as_double((long long)gw2);
    }
    if (a.npart > 0) eps_part_publish(m, f, a.pub, &m, &f);
    if (a.gdev && threadIdx.x == 0) gate_decide(a, a.dt, a.dh, m, (int)f, a.npart > 0);
    return;
  }
  const int ntx = (a.n1 + TX - 1) / TX;
  int tile, chunk, kb, ke;
  bool bw, bshort;
  pft_zplan_chunk((int)blockIdx.x, a.ntile, a.nchunk, a.nbw, a.bends, a.c0, a.nint, &tile, &chunk, &bw, &bshort);
  const int x0 = (tile % ntx) * TX, y0 = (tile / ntx) * TY;
  // threads beyond the WX x TY tile (256 > WX * TY) shadow the tile's last thread: the same loads
  // and LDS writes (same values to the same slots), no global stores
  const int tt = min((int)threadIdx.x, WX * TY - 1);
  const int tx = tt % WX, ty = tt / WX;
  const int i0 = x0 + 2 * tx, j = y0 + ty;
  const bool active = (i0 < a.n1) && (j < a.n2) && (int)threadIdx.x < WX * TY;
  const long po = (long)(j < a.n2 ? j : a.n2 - 1) * a.n1 + (i0 < a.n1 ? i0 : a.n1 - 2);
  pft_zplan_planes(chunk, bshort, a.n3, a.k_begin, a.k_end, a.kz, a.kspan, &kb, &ke);
  const int lo = (ty + 1) * LW + 2 + 2 * tx;

  const int t = threadIdx.x;
  const bool hact = t < 3 * NH;
  const int hf = hact ? t / NH : 0, h = hact ? t % NH : 0;
  int hr, hcp;
  if (h < LW / 2) { hr = 0; hcp = h; }
  else if (h < LW) { hr = LH - 1; hcp = h - LW / 2; }
  else { const int q = h - LW; hr = 1 + q / 2; hcp = (q & 1) ? LW / 2 - 1 : 0; }
  const int hi = x0 - 2 + 2 * hcp, hj = y0 + hr - 1;
  // Walls in LDS: a halo pair outside the domain holds the mirror image the reference's ghost
  // fill puts there (equation.c:137-174: ghost -1-m = interior m), so the stencil reads its x/y
  // neighbours without selects.  Pair (-2,-1) = (v1, v0): pair (0,1) swapped; pair (n1, n1+1) =
  // (v[n1-1], v[n1-2]): pair (n1-2, n1-1) swapped (held in natural order, below); rows -1 / n2 =
  // rows 0 / n2-1.
  const long hp = (long)(hj < 0 ? 0 : (hj >= a.n2 ? a.n2 - 1 : hj)) * a.n1 +
                  (hi < 0 ? 0 : (hi >= a.n1 ? a.n1 - 2 : hi));
  const int hl = hr * LW + 2 * hcp;
  // An inactive pair just right of the domain (partial tile) is the mirror of the last pair.  Every
  // pair, mirrored ones included, is stored in natural order (16-byte stores), and the thread next
  // to a mirrored pair reads its other cell instead: (-2, -1) holds (v0, v1), cell -1 = its even
  // cell; (n1, n1 + 1) holds (v[n1-2], v[n1-1]), cell n1 = its odd cell (xma / xpa: offsets of the
  // x-neighbour reads).  (Round 3 stored mirrored pairs as two 8-byte halves at exchanged offsets:
  // 2-way LDS bank conflicts)
  const int xma = i0 - 2 < 0 ? 1 : 0, xpa = i0 + 2 >= a.n1 ? 1 : 0;

  double m = 0.0;
  bool nf = false;
  dbl2 zm[3], zc[3], zp[3];
  constexpr bool FLUX = MODE != 10 && MODE != 11;
  // face reuse (rhs_cell_f) in every stage; stage 5 holds two planes of combine operands beside
  // the z-face carry (235 VGPRs, no spills)
  // two-deep z pipeline (stages 1-4): the raw operands of plane k+2 are loaded while plane k is
  // computed (the stage input of plane k+1 is its z+1 neighbour, so a one-deep pipeline waits for
  // its loads before the stencil).  It costs the operand registers: 2 waves/SIMD.  Measured at
  // 400^3: stages 3-4 0.258 vs 0.288-0.296 ms, stage 1 0.158 vs 0.166, stage 2 0.217 vs 0.222.
  constexpr bool DEEP = STAGE >= 1 && STAGE <= 4;
  Ops pn[3], ph;                       // DEEP: operands of plane k+1 (centre, halo pair)
  FaceT fz[2];                         // z-face below plane k of each cell of the pair
  // stage 2 stores S = K1 + K2 (stage 3's input combine, hybrid2.c:408), K1 carried in registers
  // (re-loading it one plane later measured 4% slower)
  constexpr bool SUM2 = STAGE == 2;
  dbl2 s2c[3], s2n[3];                 // SUM2: K1 of planes k and k+1 (the stored sum's operand)
  // stage 5 keeps x, K1, K4 and the K1/K3/K4 part of the error norm of planes k and k+1
  // (re-loading them one plane later misses the 4 MiB L2: 0.52 vs 0.65 ms at 400^3)
  dbl2 cx[3], ck1[3], ck4[3], cE[3], nx[3], nk1[3], nk4[3], nE[3];
  int cur = 0;
  const long o0 = (long)(kb + 1) * a.plane + po;
  const bool wlo = kb == 0 && !a.has_below;
  const long ob = wlo ? o0 : o0 - a.plane;
  Ops cop[3], bop[3], hop;
  if (kb < ke) {
#pragma unroll
    for (int q = 0; q < 3; ++q) load_ops<STAGE, GLS>(a, q, o0, cop[q]);
#pragma unroll
    for (int q = 0; q < 3; ++q) load_ops<STAGE, GLS>(a, q, ob, bop[q]);
    load_ops<STAGE, GLS>(a, hf, (long)(kb + 1) * a.plane + hp, hop);
  }
  if (a.gate) {
    if (gw0 != a.gseq) return;         // rejected (or NaN): leave before any store
    const double gt = __longlong_as_double((long long)gw1), gh = __longlong_as_double((long long)gw2);
    gate_scalars<STAGE>(a, c, gt, gh);
    a.dt = gt;
    a.dh = gh;
  }
  if (kb < ke) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      zc[q] = stage_in<STAGE, GLS>(a, q, cop[q]);
      if constexpr (SUM2) s2c[q] = cop[q].k1;
      if (STAGE == 5) keep5<GLS>(q, cop[q], cx[q], ck1[q], ck4[q], cE[q]);
      zm[q] = wlo ? zc[q] : stage_in<STAGE, GLS>(a, q, bop[q]);
      st2(&lds[0][q][lo], zc[q]);
    }
    if (hact) st2(&lds[0][hf][hl], stage_in<STAGE, GLS>(a, hf, hop));
    // the DEEP look-ahead after those loads are consumed, as before: the loop then starts with
    // only the look-ahead in flight (with it issued together with the rest, the compiler's wait
    // placement serialised the loop's own look-ahead: stage 1 at 400^3 0.149 -> 0.175 ms)
    if constexpr (DEEP) {
      if (!((kb == a.n3 - 1) && !a.has_above)) {
#pragma unroll
        for (int q = 0; q < 3; ++q) load_ops<STAGE, GLS>(a, q, o0 + a.plane, pn[q]);
      }
      if (hact && kb + 1 < ke) load_ops<STAGE, GLS>(a, hf, (long)(kb + 2) * a.plane + hp, ph);
    }
    // the z-face below the chunk's first plane; later planes inherit it from the plane below
#pragma unroll
    for (int s = 0; s < 2; ++s)
      fz[s] = face_of(c, zm[1][s], zm[2][s], zm[0][s], zc[1][s], zc[2][s], zc[0][s], FLUX);
    __syncthreads();
  }
  for (int k = kb; k < ke; ++k) {
    const long o = (long)(k + 1) * a.plane + po;
    const bool top = (k == a.n3 - 1) && !a.has_above;
    const bool more = k + 1 < ke;
    // z+1 neighbours: the stage input of plane k+1 (interior, or the exchanged ghost plane)
    if (!top) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if constexpr (DEEP) {
          zp[q] = stage_in<STAGE, GLS>(a, q, pn[q]);
          if constexpr (SUM2) s2n[q] = pn[q].k1;
        } else {
          Ops nop;
          load_ops<STAGE, GLS>(a, q, o + a.plane, nop);
          zp[q] = stage_in<STAGE, GLS>(a, q, nop);
          if constexpr (SUM2) s2n[q] = nop.k1;
          if (STAGE == 5) keep5<GLS>(q, nop, nx[q], nk1[q], nk4[q], nE[q]);
        }
      }
    }
    dbl2 hv = {0.0, 0.0};
    if (more) {
#pragma unroll
      for (int q = 0; q < 3; ++q) st2(&lds[cur ^ 1][q][lo], zp[q]);
      if (hact) {
        if constexpr (DEEP) {
          hv = stage_in<STAGE, GLS>(a, hf, ph);
        } else {
          Ops tmp;
          load_ops<STAGE, GLS>(a, hf, (long)(k + 2) * a.plane + hp, tmp);
          hv = stage_in<STAGE, GLS>(a, hf, tmp);
        }
      }
    }
    if constexpr (DEEP) {
      // operands of plane k+2 (and its halo pair), in flight during the stencil of plane k
      if (more) {
        if (!((k + 1 == a.n3 - 1) && !a.has_above)) {
#pragma unroll
          for (int q = 0; q < 3; ++q) load_ops<STAGE, GLS>(a, q, o + 2 * a.plane, pn[q]);
        }
        if (hact && k + 2 < ke) load_ops<STAGE, GLS>(a, hf, (long)(k + 3) * a.plane + hp, ph);
      }
    }
    if (top) {                         // top wall (uniform): mirror p, gl; Dirichlet u (equation.c:175-183)
#pragma unroll
      for (int q = 1; q < 3; ++q) zp[q] = zc[q];
      zp[0] = dbl2{a.T_top, a.T_top};
    }
    double du[2], dp[2];
    FaceT fx;                          // the x-face between the pair's two cells
    // the y neighbours of both cells as one 16-byte LDS read per neighbouring pair (consecutive
    // lanes: no bank conflicts, where two 8-byte reads at a 16-byte lane stride conflict 2-way)
    dbl2 ym2[3], yp2[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      ym2[q] = ld2(&lds[cur][q][lo - LW]);
      yp2[q] = ld2(&lds[cur][q][lo + LW]);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      Col col[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double* L = lds[cur][q];
        const double cen = zc[q][s];
        col[q].c = cen;
        // x/y neighbours straight from LDS: the walls' mirror values are in the halo
        col[q].xm = s == 0 ? L[lo - 1 - xma] : zc[q][0];
        col[q].xp = s == 0 ? zc[q][1] : L[lo + 2 + xpa];
        col[q].ym = ym2[q][s];
        col[q].yp = yp2[q][s];
        col[q].zm = zm[q][s];
        col[q].zp = zp[q][s];
      }
      const double un = a.noise ? zc[0][s] + a.noise[(long)k * a.plane + po + s] : zc[0][s];
      const FaceT fxm =
          s == 0 ? face_of(c, col[1].xm, col[2].xm, col[0].xm, col[1].c, col[2].c, col[0].c, FLUX) : fx;
      FaceT fzp;
      rhs_cell_f<MODE>(c, col[0], col[1], col[2], un, fxm, fz[s], fx, fzp, du[s], dp[s]);
      fz[s] = fzp;
    }
    if (more && hact) st2(&lds[cur ^ 1][hf][hl], hv);
    if (active) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (q == 2 && STAGE != 0 && (GLS || STAGE <= 4)) continue;   // gl's K's: literal zeros, never stored
        const dbl2 K = q == 0 ? dbl2{du[0], du[1]} : (q == 1 ? dbl2{dp[0], dp[1]} : dbl2{0.0, 0.0});
        const long e = q * a.fs + o;
        if (SUM2) {
          dbl2 S;
          const dbl2 k1c = s2c[q];
#pragma unroll
          for (int s = 0; s < 2; ++s) S[s] = k1c[s] + K[s];   // K1 + K2, hybrid2.c:408
          st2(a.kout + e, S);
        } else if (STAGE <= 4) {
          st2(a.kout + e, K);
        } else {
          // the combine operands of plane k, kept in registers since they were loaded
          // gl (q = 2): K1, K4 and the K part of the error norm are the literal zeros of dgl
          // (equation.c:731), so they are not carried in registers
          constexpr dbl2 zero2 = {0.0, 0.0};
          const bool z2 = q == 2;
          const dbl2 ox = cx[q], ok1 = z2 ? zero2 : ck1[q], ok4 = z2 ? zero2 : ck4[q];
          dbl2 oE = cE[q];
          if (z2) {
#pragma unroll
            for (int s = 0; s < 2; ++s) oE[s] = 0.2 * 0.0 - 0.9 * 0.0 + 0.8 * 0.0;   // :521 prefix
          }
          dbl2 r;
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const double em = q == 0 ? a.em0 : (q == 1 ? a.em1 : a.em2);
            const double ev = em * fabs(oE[s] - 0.1 * K[s]);                                    // :521
            if (ev > m) m = ev;                                                               // NaN never wins
            nf |= !isfinite(ev);
            r[s] = ox[s] + a.coef * (0.5 * (ok1[s] + K[s]) + 2.0 * ok4[s]);                  // :667
          }
          if (!(q == 2 && a.gl_keep)) st2(a.out + e, r);
        }
      }
    }
    __syncthreads();
    cur ^= 1;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      zm[q] = zc[q];
      zc[q] = zp[q];
      if constexpr (SUM2) s2c[q] = s2n[q];
      if (STAGE == 5) { cx[q] = nx[q]; ck1[q] = nk1[q]; ck4[q] = nk4[q]; cE[q] = nE[q]; }
    }
  }

  if (STAGE == 5) {
    __shared__ double red[PFT_FBLOCK / 64];
    __shared__ int rnf[PFT_FBLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(m, off, 64);
      if (ov > m) m = ov;
    }
    const int anynf = __any(nf);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      red[w] = m;
      rnf[w] = anynf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double bm = red[0];
      int bnf = rnf[0];
      for (int q = 1; q < PFT_FBLOCK / 64; ++q) {
        if (red[q] > bm) bm = red[q];
        bnf |= rnf[q];
      }
      if (a.part) eps_store_part(a.part, bm, bnf);
      else eps_arrive(bm, bnf, a.shards, a.eps_bits, a.nonfinite, a.pub, a.pub_count);
    }
  }
  if (bw) {
    // an inline boundary workgroup (as merson_pair's): stores done, L2 written back, counted.  (A
    // gated launch, which may leave before its stores, never runs inline: run_stage)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      __hip_atomic_fetch_add(a.bdone, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------------------------------
// the pair kernel: two consecutive Merson stages (2+3, or 4+5) in ONE z-march.
//
// Stage B's input at a cell is a pointwise combine of x, the K's and stage A's K there
// (hybrid2.c:408 / :449), so stage B's 7-point stencil at the tile needs stage A's K on the tile
// plus a one-cell ring, and stage A's stencil there needs stage A's input on a two-cell ring.  A
// workgroup recomputes stage A on its ring (the neighbouring workgroups compute the same cells
// with the same operands in the same order: the same bits) and never stores it: K2 and K4 do
// not exist in HBM, and neither stage re-reads x and the K's the other one read.  Per cell-step:
//   stages 2, 3 apart: (5 + 2) + (5 + 2) = 14 doubles -> pair 2+3: x, K1 in, K3 out = 7
//   stages 4, 5 apart: (7 + 2) + (9 + 2) = 20 doubles -> pair 4+5: x, K1, K3 in, x(t+h) out = 9
// so the step (speculative stage 1 + the two pairs) moves 21 instead of 39 doubles per cell.
//
// Workgroup (PFT_PBLOCK threads): an R0 tile of tx x ty cells (tx even) is stage B's output.
// Thread (px, py) holds the cell pair (x0 - 2 + 2 px, x0 - 1 + 2 px) of row y0 - 2 + py, for px
// in [0, tx/2 + 2) and py in [0, ty + 4): the tile plus a two-cell ring (R2).  Every thread loads
// its pair's operands and writes stage A's input into LDS (plane ring lA); threads of rows
// 1..ty+2 (the tile plus a one-cell ring, R1) evaluate stage A at their pair and write stage B's
// input into LDS (plane ring lB); threads of the tile evaluate stage B.  A position outside the
// domain (walls) holds the mirror image the reference's ghost fill puts there (equation.c:137-174:
// ghost -1-m = interior m): its thread loads the mirrored in-domain pair ("acting" pair), stores
// it into LDS with its halves exchanged when mirrored in x, and evaluates stage A exactly as the
// acting pair's own thread does -- so the mirrored stage-B input is the reference's bit for bit.
// z neighbours of both levels are read from the plane rings (own pair: written by the thread
// itself; x/y neighbours: written one iteration earlier, behind the barrier).
//
// Positions beyond the 512 threads (round 6, the 40 x 20 tile: 22 x 24 = 528 positions).  The
// last ring row (py = ty + 3) is only read, as the y neighbours of stage A's last row; its
// positions past thread 511 (at most PFT_PAIR_NEX, all in that row) are loaded by the last lanes
// of the last wave, whose own positions are load-only (ring rows 0 and ty + 3): such a lane never
// reads plane mm's operand set (rc: stage B's input and lO belong to the other rows) and is done
// with plane mm + 1's (rn) after the top of the step, so of the three rotating PairRaw sets two
// hold nothing it needs.  It loads the extra position's operands into rn with ordinary loads, one
// step ahead, and a step later -- the set is rc by then -- combines them into stage A's input and
// stores it into lA: no register the allocation does not already hold, no staging in LDS.  (Round 6
// staged them by LDS DMA, global_load_lds_dwordx4 through hand-ordered asm, on the premise that
// the kernel has no register to spare at 256 VGPRs; that cost pair 4+5 about 4%: DESIGN.md
// section 8.00000.)
// The taller tile evaluates stage B on 400 positions instead of 380 with the same wave-phases per
// plane, n2 = 200 / 400 is cut into 10 / 20 tile rows with no idle row (19-row tiles: 11 / 22, the
// last one half empty), and 400^3 runs its 50 tiles x 5 z-chunks in one round of 250 workgroups
// (55 x 9 in two rounds before): DESIGN.md section 8.0.
#define PFT_PBLOCK 512
#define PFT_PAIR_NEX 16
// LDS layout of a field plane: the positions' cell pairs side by side (16 bytes a slot, PairLds
// below), position (px, py) at slot PFT_PAIR_PADP + py LWP + px.  (The layout with the even and
// odd cells in two halves, conflict-free 8-byte accesses, was removed in round 5: PairLds.)
#define PFT_PAIR_PADP 2         // slots before / after the positions of each half: the discarded
                                // outer cell of a ring pair reads one slot beyond its row
#define PFT_PAIR_H 532          // pair slots of a stage-A field plane (rows 0..ty+3 at the row pitch)
#define PFT_PAIR_HB 488         // slots of a stage-B plane in the interleaved layout (rows 1..ty+2)
// The row pitch LWP (pairs) is a template parameter, a compile-time constant so that every LDS
// access is a per-lane base + an immediate offset: 22 (tiles up to 40 cells wide, 20 rows) or 12
// (up to 20 cells wide, 38 rows: n1 = 100 in 5 tiles of 20 where 40-wide tiles leave a sixth idle)
// measured crossover (profiles/r05_pair_threshold.txt, stage launches against pair kernels forced):
// 128^3 (2048 cells per CU) -10%, 136^3 (2456) -1.4%, 144^3 (2916) +16%, 152^3 (3429) +18%, 160^3
// (4000) +9%, 200^3 (7.8 Ki) +7-9%
#define PFT_PAIR_MIN_CELLS_PER_CU 2560

struct PairArgs {
  const double* x;
  const double* k1;
  const double* k3;     // pair 4+5 only
  double* out;          // pair 2+3: K3 (u, p); pair 4+5: x(t+h) (u, p; gl unless gl_keep)
  const double* noise;  // u_noise [k][j][i] or null
  unsigned long long* eps_bits;
  unsigned int* nonfinite;
  unsigned long long* pub;   // in-kernel publication of the error norm (as merson_fused<5>)
  unsigned int* pub_count;
  EpsShard* shards;    // the error norm's per-shard accumulators (eps_arrive)
  unsigned long long* part;   // deferred publication: this launch's workgroup partials (eps_store_part)
  long fs;
  int n1, n2, n3, plane;
  int has_below, has_above;   // z-neighbours: stage A also runs on the ghost plane next to each,
                              // from the two-plane halo (ghost + far ghost planes, pft_slab_far)
  int k_begin, k_end, kz, ntile, nchunk, ntx;
  int kspan;            // planes a chunk runs from its start (kz; 2 for the two-plane boundary launch)
  // inline boundary (PFT_K_INLINE, PFT_K_ENDS_FIRST; pft_zplan.h): the grid's first nbw workgroups
  // produce the planes the exchange sends, each adding one to *bdone once they are written back
  int nbw, bends, c0, nint;
  unsigned long long* bdone;
  int tx, ty;           // R0 tile: tx cells (even) x ty rows
  double T_topA, T_topB;   // Dirichlet u above the top plane at the two stage times
  double cinA, cinB;    // stage-input coefficients: h/3, h/6 (2+3); h/8, h (4+5)
  double coef;          // x(t+h) coefficient h/3 (4+5)
  double em0, em1;
  // gl's K's are the literal zeros of dgl (equation.c:731,874), so every gl term of the step is a
  // per-launch constant the host evaluates with the reference's expression (pair_gl_consts):
  // stage A's and stage B's gl input are glA + x and glB + x, x(t+h) of gl is x + glX, and gl's
  // error-norm term is evgl.  GLX kernels (gl_static, or gl_keep: x's gl holds no -0.0 or NaN and
  // the coefficients are finite) read gl's inputs straight from x: glA + x == x bit for bit there.
  double glA, glB, glX, evgl;
  int gl_keep;
};
// byte offset of the kernel's second argument (pft_consts) in the kernarg segment
static constexpr unsigned PFT_PAIR_COFF =
    (unsigned)((sizeof(PairArgs) + alignof(pft_consts) - 1) / alignof(pft_consts) * alignof(pft_consts));

// The z-loop re-reads the kernel arguments (PairArgs, pft_consts) from the kernarg segment with
// scalar loads at each of its three phases (PFT_PAIR_BIND: the pointer is laundered through an
// empty asm, so the loads cannot be hoisted out of the loop).  Kept live across the whole loop,
// the ~25 model constants, the array bases and the step coefficients needed ~190 SGPRs: ~90 were
// spilled into VGPR lanes and re-read by ~160 v_readlane per iteration (pair 4+5 0.519 -> 0.486 ms
// at 400^3; pair 2+3 0.408 -> 0.403 ms).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) char* pft_kptr;
#define PFT_PAIR_BIND(A, C)                                                                  \
  pft_kptr kq_##A = kbase;                                                                  \
  asm volatile("" : "+s"(kq_##A));                                                          \
  const PairArgs& A = *(const __attribute__((address_space(4))) PairArgs*)kq_##A;           \
  const pft_consts& C = *(const __attribute__((address_space(4))) pft_consts*)(kq_##A + PFT_PAIR_COFF)
#else
#define PFT_PAIR_BIND(A, C) \
  const PairArgs& A = a;    \
  const pft_consts& C = c
#endif

// operands of one cell pair: x (u, p, gl), K1 and K3 (u, p; gl's K's are the literal zeros of
// dgl, equation.c:731,874)
struct PairRaw {
  dbl2 x[3], k1[2], k3[2];
};

// 16-byte load / store at a byte offset from a wave-uniform base: the base stays in SGPRs and the
// per-lane offset is one 32-bit VGPR for every array (global_load saddr + voffset), instead of a
// 64-bit address per array and plane (pft_slab_pair_ok: a field is < 4 GiB)
__device__ __forceinline__ dbl2 ldb(const double* base, unsigned bo)
{
  return *reinterpret_cast<const dbl2*>(reinterpret_cast<const char*>(base) + bo);
}
__device__ __forceinline__ void stb(double* base, unsigned bo, dbl2 v)
{
  *reinterpret_cast<dbl2*>(reinterpret_cast<char*>(base) + bo) = v;
}

// operands of plane m in [-2, n3 + 1] (interior 0..n3-1; -1 and n3 the ghost planes, -2 and n3+1
// the far ghost planes of the two-plane halo) at byte offset bo = pbo(m).  The PairArgs pointers
// are the buffers' pointers minus one plane (run_pair): field q holds plane m at q fs + (m + 2)
// plane from there, so every offset is unsigned.  gl's x is loaded only where an input needs it.
template <int SA, bool GL = true>
__device__ __forceinline__ void pair_load(const PairArgs& a, unsigned bo, PairRaw& r)
{
#pragma unroll
  for (int q = 0; q < (GL ? 3 : 2); ++q) r.x[q] = ldb(a.x + q * a.fs, bo);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    r.k1[q] = ldb(a.k1 + q * a.fs, bo);
    if (SA == 4) r.k3[q] = ldb(a.k3 + q * a.fs, bo);
  }
}

// stage A's input (stage 2: hybrid2.c:388; stage 4: :428) -- the expressions of stage_in; gl:
// glA + x (the combine of its literal-zero K's, a per-launch constant), x itself under GLX
template <int SA, bool GLX>
__device__ __forceinline__ dbl2 pair_in_A(const PairArgs& a, int q, const PairRaw& r)
{
  if (q == 2) {
    if (GLX) return r.x[2];
    return dbl2{a.glA + r.x[2][0], a.glA + r.x[2][1]};
  }
  const dbl2 k1 = r.k1[q < 2 ? q : 0];
  const dbl2 k3 = r.k3[q < 2 ? q : 0];
  dbl2 v;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (SA == 2) v[s] = k1[s] * a.cinA + r.x[q][s];
    else v[s] = (k1[s] + 3.0 * k3[s]) * a.cinA + r.x[q][s];
  }
  return v;
}

// stage B's input from the operands and stage A's K at the cell (stage 3: (K1 + K2) h/6 + x,
// hybrid2.c:408; stage 5: (0.5 K1 - 1.5 K3 + 2 K4) h + x, :449)
template <int SA, bool GLX>
__device__ __forceinline__ dbl2 pair_in_B(const PairArgs& a, int q, const PairRaw& r, dbl2 KA)
{
  if (q == 2) {
    if (GLX) return r.x[2];
    return dbl2{a.glB + r.x[2][0], a.glB + r.x[2][1]};
  }
  const dbl2 k1 = r.k1[q < 2 ? q : 0];
  const dbl2 k3 = r.k3[q < 2 ? q : 0];
  dbl2 v;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (SA == 2) v[s] = (k1[s] + KA[s]) * a.cinB + r.x[q][s];
    else v[s] = (0.5 * k1[s] - 1.5 * k3[s] + 2.0 * KA[s]) * a.cinB + r.x[q][s];
  }
  return v;
}

// A field plane of a ring holds the positions' cell pairs side by side (slot p: doubles 2p, 2p + 1),
// mirrored positions in natural order (the neighbour reading one takes its other cell).  A cell read
// on its own is an 8-byte access at a 16-byte lane stride (2-way bank conflicts), so pair_rhs reads
// the y neighbours of both cells as one 16-byte access per neighbouring pair (consecutive lanes,
// conflict-free).  Measured against it and removed (A/B on one box each, 400^3;
// profiles/r04b_ab_small_grids_and_layouts.txt): the even and odd cells in two
// halves (every access conflict-free, no 16-byte accesses, more address registers): pair 2+3
// 0.357-0.359 ms against 0.352-0.356, pair 4+5 0.416-0.424 against 0.409-0.411 (a spill); the y
// neighbours as two 8-byte reads: pair 2+3 0.362-0.365, pair 4+5 0.410-0.415.
#define PFT_PAIR_OPN 400      // stage-B positions of a tile ((tx/2) ty, at most 400: pair_geometry_ok)
struct PairLds {
  __device__ static __forceinline__ dbl2 ld(const double* L, int p) { return ld2(L + 2 * p); }
  __device__ static __forceinline__ void st(double* L, int p, dbl2 v) { st2(L + 2 * p, v); }
  __device__ static __forceinline__ double cell(const double* L, int p, int s) { return L[2 * p + s]; }
};

// the RHS of one cell pair (du, dp of both cells): centre zc, z neighbours zm / zp, x/y
// neighbours from the LDS field planes L[q] around slot p (even / odd halves, row pitch LWP); the
// x-face between the pair's cells is evaluated once and the z-face below is carried in fz
// (rhs_cell_f, bit-exact), as in merson_fused
// (HN: field 2's x/y neighbours come from hn, read by pair_nbr2 ahead of the call, and L2 is not
// touched: the staggered stage B, whose gl plane in lA is being overwritten while it runs)
struct PairNbr {
  dbl2 ym, yp;      // the pairs one row below / above
  double xm, xp;    // the cells left of the even / right of the odd cell
};
template <int LWP>
__device__ __forceinline__ PairNbr pair_nbr2(const double* L2, int p, int xmc, int xpc)
{
  using LD = PairLds;
  return PairNbr{LD::ld(L2, p - LWP), LD::ld(L2, p + LWP), LD::cell(L2, p - 1, xmc), LD::cell(L2, p + 1, xpc)};
}
template <int MODE, int LWP, bool HN = false>
__device__ __forceinline__ void pair_rhs(const pft_consts& c, const double* L0, const double* L1, const double* L2,
                                         int p, int xmc, int xpc, const dbl2* zm, const dbl2* zc, const dbl2* zp,
                                         const double* nz, FaceT* fz, double* du, double* dp,
                                         const PairNbr* hn = nullptr)
{
  constexpr bool FLUX = MODE != 10 && MODE != 11;
  using LD = PairLds;
  const double* L[3] = {L0, L1, L2};
  // the y neighbours of both cells as one 16-byte read per neighbouring pair (consecutive lanes,
  // conflict-free) instead of two 8-byte reads at a 16-byte lane stride
  dbl2 ym2[3], yp2[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (HN && q == 2) {
      ym2[q] = hn->ym;
      yp2[q] = hn->yp;
      continue;
    }
    ym2[q] = LD::ld(L[q], p - LWP);
    yp2[q] = LD::ld(L[q], p + LWP);
  }
  FaceT fx;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    Col col[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double cen = zc[q][s];
      col[q].c = cen;
      // the cell of the pair to the left / right next to this pair: its odd / even cell, or the
      // other one where that slot holds a mirrored position in natural order (xmc / xpc)
      if (HN && q == 2) {
        col[q].xm = s == 0 ? hn->xm : zc[q][0];
        col[q].xp = s == 0 ? zc[q][1] : hn->xp;
      } else {
        col[q].xm = s == 0 ? LD::cell(L[q], p - 1, xmc) : zc[q][0];
        col[q].xp = s == 0 ? zc[q][1] : LD::cell(L[q], p + 1, xpc);
      }
      col[q].ym = ym2[q][s];
      col[q].yp = yp2[q][s];
      col[q].zm = zm[q][s];
      col[q].zp = zp[q][s];
    }
    const double un = nz ? zc[0][s] + nz[s] : zc[0][s];
    const FaceT fxm =
        s == 0 ? face_of(c, col[1].xm, col[2].xm, col[0].xm, col[1].c, col[2].c, col[0].c, FLUX) : fx;
    FaceT fzp;
    rhs_cell_f<MODE>(c, col[0], col[1], col[2], un, fxm, fz[s], fx, fzp, du[s], dp[s]);
    fz[s] = fzp;
  }
}

// Thread (virtual position index v) -> position (px, py) of a tile of bw = tx/2 stage-B pairs x ty
// rows (round 6), for tiles with positions beyond the threads: whole rows of the R2 tile, each
// row contiguous (wp2 = bw + 2 pairs, so every load and store of a row is one run, as row-major),
// but in the order: stage B's rows 2 .. ty + 1 first, then stage A's ring rows 1 and ty + 2, then
// the load-only rows 0 and ty + 3 -- the last of them beyond the threads (pair_geometry_ok: at most
// PFT_PAIR_NEX, all in row ty + 3).  With 22-pair rows (40 x 20 tile) stage B's 20 rows end at
// thread 439, so the last wave (448 .. 511) holds ring rows only and skips stage B: its SIMD runs 3
// wave-phases a plane where the others run 4, and the extra positions' combine and LDS stores ride
// in that slack instead of delaying the barrier.  The threads that take an extra position, the
// last NPOS - 512 of the order, lie in the load-only rows (NPOS - 512 <= tx/2 + 2, since rows
// 0 .. ty + 2 fit the threads: pair_geometry_ok), which is what frees their registers.  (Stage-B positions compacted to threads 0 .. 399, ring
// columns after them, did the same for pair 2+3 but cost pair 4+5 9%: its rows no longer one run;
// profiles/r06_ab_pair_tile.txt.)  Row-major from row 0 for tiles without extra positions.
__device__ __forceinline__ void pair_pos(int v, int bw, int ty, int& px, int& py)
{
  const int wp2 = bw + 2;
  if (v < ty * wp2) {                                  // stage B's rows
    py = 2 + v / wp2;
    px = v % wp2;
    return;
  }
  v -= ty * wp2;
  if (v < 2 * wp2) {                                   // stage A's ring rows
    py = v < wp2 ? 1 : ty + 2;
    px = v < wp2 ? v : v - wp2;
    return;
  }
  v -= 2 * wp2;                                        // load-only rows
  py = v < wp2 ? 0 : ty + 3;
  px = v < wp2 ? v : v - wp2;
}

template <int N>
using pft_ic = std::integral_constant<int, N>;

// The stagger of the pair kernels' wave halves.  The two waves of a
// SIMD, w and w + 4, run the same plane step between the same two barriers; with the stagger the
// late half (waves 4-7) passes a step's barrier between stage A and stage B instead of at the
// step's end, so its stage B runs in the next barrier interval, beside the early half's top and
// stage A.  Every wave still passes one barrier per step and runs the same text in the same order.
// Which instances keep it (measured, 400^3 and 200^3, profiles/f14_stagger_ab.txt): pair 2+3 on
// the 22-pair pitch in calc_modes 0 and 1, +1.0% and +1.4% on the step.  Pair 4+5 lost 1.4% with
// it (tied at best, with a static priority), calc_mode 2 lost 3.6% and the 12-pair pitch 3% at
// 200^3: they keep the barrier at the step's end, and so do modes 10 and 11, which no benchmark
// measures.
// -DPFT_PAIR_STAGGER=0: every wave at the step's end, as before (A/B); a bit mask otherwise
// (1: pair 2+3, 2: pair 4+5, 4: the 12-pair pitch too, 8: every calc_mode).  -DPFT_PAIR_STAGGER_ODD=1: the odd waves
// as the late half (the control: partners are w / w + 4, and it lost).
// -DPFT_PAIR_PRIO: the s_setprio scheme of staggered kernels, 0: the per-phase flips (kept),
// 1: none, 2: one static s_setprio 1 for the late half.
#ifndef PFT_PAIR_STAGGER
#define PFT_PAIR_STAGGER 1
#endif
#ifndef PFT_PAIR_STAGGER_ODD
#define PFT_PAIR_STAGGER_ODD 0
#endif
#ifndef PFT_PAIR_PRIO
#define PFT_PAIR_PRIO 0
#endif
constexpr bool pair_stagger(int SA, int MODE, bool GLX, int LWP)
{
  (void)GLX;
  return (PFT_PAIR_STAGGER & (SA == 2 ? 1 : 2)) && (LWP == 22 || (PFT_PAIR_STAGGER & 4)) &&
         (MODE == 0 || MODE == 1 || (PFT_PAIR_STAGGER & 8));
}

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Warray-bounds"
template <int SA, int MODE, bool GLX, int LWP>
__global__ __launch_bounds__(PFT_PBLOCK) __attribute__((amdgpu_waves_per_eu(2))) void merson_pair(PairArgs a,
                                                                                                   pft_consts c)
{
  constexpr bool FLUX = MODE != 10 && MODE != 11;
  constexpr dbl2 zero2 = {0.0, 0.0};
  using LD = PairLds;
#if defined(__HIP_DEVICE_COMPILE__)
  const pft_kptr kbase = (pft_kptr)__builtin_amdgcn_kernarg_segment_ptr();
#endif
  // (the stage-B ring holds rows 1..ty+2 only: PFT_PAIR_HB slots)
  // OPL (pair 4+5 with GLX): stage B's gl input is x's gl, which
  // lA already holds for the same plane -- lB keeps u and p only and stage B reads gl from lA
  // (its z neighbour below from a register: lA's slot of that plane is overwritten by then).  The
  // 22 KiB this frees, with the 22 KiB left over, hold the operands of stage B's outputs (x, K1,
  // K3 of u and p at each stage-B position, 36 KiB): written when they arrive for stage A, read
  // back one plane later by the same thread, instead of their second load from beyond L2 (the
  // re-load: pair 4+5 1.5% slower, 1.80x the algorithmic bytes beyond L2 against 1.11x).
  // (GLB: the same gl sharing in pair 2+3, whose ZREG registers hold stage A's gl inputs at the
  // thread's own position: stage B's gl centre and z neighbours come from there; without it pair
  // 2+3 took 0.341-0.344 against 0.337-0.340 ms)
  constexpr bool GLB = GLX;
  constexpr bool OPL = SA == 4 && GLB;
  constexpr int NBQ = GLB ? 2 : 3;   // lB's fields
  __shared__ __attribute__((aligned(16))) double lA[3][3][2 * PFT_PAIR_H];
  __shared__ __attribute__((aligned(16))) double lB[3][NBQ][2 * PFT_PAIR_HB];
  // (without OPL a 1 x 1 placeholder: its accesses below sit in a branch that is constant-false
  // there, which -Warray-bounds flags per instantiation; an if constexpr would drop the placeholder
  // and shift the LDS layout of every other kernel)
  __shared__ __attribute__((aligned(16))) dbl2 lO[OPL ? 6 : 1][OPL ? PFT_PAIR_OPN : 1];
  // the extra positions' acting-pair offsets, set once (the tile's corner x0, y0 is not kept live
  // across the loop for them: pair 4+5 has no register or SGPR to spare, and recomputing the corner
  // takes the tile's index through xcd_remap, where this is one LDS read)
  __shared__ unsigned lXa[PFT_PAIR_NEX];

  const int TX = a.tx, TY = a.ty, WP2 = TX / 2 + 2, NPOS = WP2 * (TY + 4);
  int tile, chunk, kb, ke;
  bool bw, bshort;
  pft_zplan_chunk((int)blockIdx.x, a.ntile, a.nchunk, a.nbw, a.bends, a.c0, a.nint, &tile, &chunk, &bw, &bshort);
  const int x0 = (tile % a.ntx) * TX, y0 = (tile / a.ntx) * TY;
  // threads beyond the R2 positions shadow the last one (same loads and LDS writes, no stores)
  const int tt = min((int)threadIdx.x, NPOS - 1);
  int px, py;
  if (LWP == 22 && NPOS > PFT_PBLOCK) {
    pair_pos(tt, TX / 2, TY, px, py);
  } else {
    // no extra positions: row-major over the R2 tile, as measured best there (200^3: the stage-B
    // positions first ran 8% slower, profiles/r06_ab_pair_tile.txt)
    px = tt % WP2;
    py = tt / WP2;
  }
  const int pi = x0 - 2 + 2 * px, pj = y0 - 2 + py;          // position: first cell, row
  // acting pair (in the domain): a mirrored position holds its values (x halves exchanged)
  const int ai = pi < 0 ? 0 : (pi >= a.n1 ? a.n1 - 2 : pi);
  const int aj = pj < 0 ? 0 : (pj >= a.n2 ? a.n2 - 1 : pj);
  // A position outside the domain in x holds the mirror image of its acting pair: the slot stores
  // the acting pair in natural order (16-byte stores and loads, no per-lane swap), and the
  // neighbour reading it takes the other cell (mirrored pair (-2, -1) = (v1, v0) holds (v0, v1):
  // cell -1 is its even cell; (n1, n1 + 1) holds (v[n1-2], v[n1-1]): cell n1 is its odd cell).
  auto mir = [&](int col) -> bool { const int c0 = x0 - 2 + 2 * col; return c0 < 0 || c0 >= a.n1; };
  const int pxa = (ai - x0 + 2) / 2;                          // the acting pair's column
  const int xmcA = mir(pxa - 1) ? 0 : 1, xpcA = mir(pxa + 1) ? 1 : 0;
  const int xmcB = mir(px - 1) ? 0 : 1, xpcB = mir(px + 1) ? 1 : 0;
  const unsigned apo = (unsigned)(aj * a.n1 + ai);
  // byte offset of the acting pair in plane m of a field, from the PairArgs pointers
  auto pbo = [&](int m) -> unsigned { return ((unsigned)(m + 2) * (unsigned)a.plane + apo) * 8u; };
  const int posA = PFT_PAIR_PADP + py * LWP + px;              // this position's slot in lA
  const int posB = PFT_PAIR_PADP + (py - 1) * LWP + px;        // ... in lB (rows 1..ty+2)
  const int actA = PFT_PAIR_PADP + (aj - y0 + 2) * LWP + (ai - x0 + 2) / 2;   // the acting pair in lA
  const bool isA = py >= 1 && py <= TY + 2;
  const bool isB = (int)threadIdx.x < NPOS && px >= 1 && px <= TX / 2 && py >= 2 && py <= TY + 1 &&
                   pi < a.n1 && pj < a.n2;
  const int ob = (py - 2) * (TX / 2) + px - 1;                // this stage-B position's slot in lO
  // positions beyond the threads (NPOS > PFT_PBLOCK: pair_geometry_ok puts them all in the last
  // ring row ty + 3, the tail of pair_pos's order): the last NPOS - PFT_PBLOCK threads (lanes
  // 64 - NEX .. 63 of the last wave, themselves load-only positions) load one each too, one plane
  // ahead like their own look-ahead, into the operand set that is dead for them (xload in step()),
  // and store its stage-A input into lA a step later.  Everything else about it is recomputed
  // where used from the thread index and the phase's kernel arguments (mostly scalar): the kernel
  // holds no further register for it across the loop (pair 4+5 is at 256 VGPRs).
  auto nex = [&](const PairArgs& A) { return (A.tx / 2 + 2) * (A.ty + 4) - PFT_PBLOCK; };
  // the loaders are lanes 64 - NEX .. 63 of the last wave; inside the z-loop they are found from
  // the wave's index (one SGPR) and the lane index (mbcnt, recomputed): keeping threadIdx.x live
  // across the loop for them cost pair 4+5 a spilled VGPR
  const int wid = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  auto lane = [&]() {
    int l;  // volatile: recomputed where used, so nothing derived from it is hoisted out of the loop
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
  };
  // (only tiles wider than 20 cells have them: the 12-pair pitch compiles the extras out)
  auto is_x = [&](const PairArgs& A) { return LWP == 22 && wid == PFT_PBLOCK / 64 - 1 && lane() >= 64 - nex(A); };
  // the extra position's column (row ty + 3) and its acting pair's offset in a plane
  auto px_x = [&](const PairArgs& A) { return lane() - 64 + (A.tx / 2 + 2); };
  auto apo_x = [&](const PairArgs& A) { return lXa[lane() - (64 - nex(A))]; };
  auto pos_x = [&](const PairArgs& A) { return PFT_PAIR_PADP + (A.ty + 3) * LWP + px_x(A); };
  auto pboe = [&](const PairArgs& A, int m) -> unsigned { return ((unsigned)(m + 2) * (unsigned)A.plane + apo_x(A)) * 8u; };
  // plane m's operands of the extra position into the set r (call under is_x only)
  auto xload = [&](const PairArgs& A, int m, PairRaw& r) { pair_load<SA>(A, pboe(A, m), r); };
  // stage A's input of the extra position from its operands r into the ring slot `slot`
  auto xstore = [&](const PairArgs& A, int slot, const PairRaw& r) {
    const int pe = pos_x(A);
#pragma unroll
    for (int q = 0; q < 3; ++q) LD::st(lA[slot][q], pe, pair_in_A<SA, GLX>(A, q, r));
  };

  pft_zplan_planes(chunk, bshort, a.n3, a.k_begin, a.k_end, a.kz, a.kspan, &kb, &ke);
  const int n3 = a.n3;
  const bool wlo = !a.has_below, whi = !a.has_above;         // walls (equation.c:164-183)
  // stage-A planes [mA0, mA1]: the chunk's planes and one on each side -- at a slab interface
  // the ghost plane (the neighbour's boundary plane, recomputed), at a wall none
  const int mA0 = kb > 0 ? kb - 1 : (wlo ? 0 : -1);
  const int mA1 = ke < n3 ? ke : (whi ? n3 - 1 : n3);
  const int mlast = min(mA1 + 1, whi ? n3 - 1 : n3 + 1);     // last stage-A input plane
  const int mfirst = wlo ? 0 : -2;                           // first stage-A input plane

  double m = 0.0;
  bool nf = false;
  // Operands in registers: those of plane mm (stage B's input), mm + 1 (landed: stage A's input)
  // and mm + 2 (in flight), rotating through R[0..2]; stage B's outputs (4+5) need plane mm - 1's
  // again: from lO (OPL), else re-loaded after stage A (in registers they would spill).
  // Plane p's LDS ring slot is (p - mA0) mod 3 and the loop is unrolled three times, so every ring
  // slot -- and with the fixed row pitch every LDS offset -- is a compile-time constant, and the
  // register rotation needs no copies.
  PairRaw R[3];
  dbl2 KA[3][2];        // stage A's K (u, p) of the last three planes, rotating with R
  // ZREG (pair 2+3, which has the registers: 218 VGPRs with it): stage A's inputs at this
  // thread's own position, plane by ring slot, kept in registers beside their LDS copies -- stage
  // A reads its z neighbours and centre from here instead of from LDS (measured: pair 2+3 0.362 ->
  // 0.354 ms, 200^3 +1.0%; profiles/r04b_ab_small_grids_and_layouts.txt ab4q).  Pair 4+5 has no
  // registers for it (256 VGPRs in use).
  constexpr bool ZREG = SA == 2;
  dbl2 IA[3][3];
  dbl2 glm = zero2;     // GLB: gl's input at this position, plane mm - 2 (stage B's z neighbour below)
  FaceT fzA[2], fzB[2];
  // the stagger (pair_stagger above): waves 4-7, the SIMDs' second waves, are the late half
  constexpr bool STG = pair_stagger(SA, MODE, GLX, LWP);
  const bool late = STG && (PFT_PAIR_STAGGER_ODD ? (wid & 1) != 0 : wid >= PFT_PBLOCK / 128);
  constexpr bool PRIOF = !STG || PFT_PAIR_PRIO == 0;   // the per-phase s_setprio flips
  if (STG && PFT_PAIR_PRIO == 2 && late) __builtin_amdgcn_s_setprio(1);

  // prologue: stage A's input of planes mA0 - 1 (if any) and mA0 into the ring (slots 2 and 0);
  // operands of mA0 kept, of mA0 + 1 in flight.  (kb >= ke: an empty chunk, which still takes
  // part in the error norm's workgroup count below)
  if (is_x(a)) {
    const int ajx = min(y0 - 2 + a.ty + 3, a.n2 - 1);
    const int aix = min(max(x0 - 2 + 2 * px_x(a), 0), a.n1 - 2);
    lXa[(int)threadIdx.x - (PFT_PBLOCK - nex(a))] = (unsigned)(ajx * a.n1 + aix);
  }
  if (kb < ke) {
    dbl2 ia0[3], iam[3];
    pair_load<SA>(a, pbo(mA0), R[0]);
    if (mA0 > mfirst) {
      PairRaw t;
      pair_load<SA>(a, pbo(mA0 - 1), t);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        iam[q] = pair_in_A<SA, GLX>(a, q, t);
        LD::st(lA[2][q], posA, iam[q]);
        if (ZREG) IA[2][q] = iam[q];
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      ia0[q] = pair_in_A<SA, GLX>(a, q, R[0]);
      LD::st(lA[0][q], posA, ia0[q]);
      if (ZREG) IA[0][q] = ia0[q];
      if (mA0 == mfirst) {
        // bottom wall: plane -1 mirrors plane 0 (equation.c:164-174), also in the ring slot of
        // plane -1, so that the z-loop reads its z neighbours without selects
        iam[q] = ia0[q];
        LD::st(lA[2][q], posA, ia0[q]);
        if (ZREG) IA[2][q] = ia0[q];
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) fzA[s] = face_of(c, iam[1][s], iam[2][s], iam[0][s], ia0[1][s], ia0[2][s], ia0[0][s], FLUX);
    if (is_x(a)) {
      // the extra position: planes mA0 - 1 and mA0 as the others' (loaded here), mA0 + 1 into
      // R[0], the first step's rc, which a load-only lane is done with (ia0 above was its last use)
      PairRaw t;
      if (mA0 > mfirst) {
        pair_load<SA>(a, pboe(a, mA0 - 1), t);
#pragma unroll
        for (int q = 0; q < 3; ++q) LD::st(lA[2][q], pos_x(a), pair_in_A<SA, GLX>(a, q, t));
      }
      pair_load<SA>(a, pboe(a, mA0), t);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const dbl2 v = pair_in_A<SA, GLX>(a, q, t);
        LD::st(lA[0][q], pos_x(a), v);
        if (mA0 == mfirst) LD::st(lA[2][q], pos_x(a), v);
      }
      if (mA0 + 1 <= mlast) xload(a, mA0 + 1, R[0]);        // consumed at the top of the first step
    }
    if (mA0 + 1 <= mlast) pair_load<SA>(a, pbo(mA0 + 1), R[1]);
    KA[2][0] = KA[2][1] = zero2;
    __syncthreads();
  }

  // one z-step: stage A at plane mm, stage B at plane mm - 1; false after the chunk's last one.
  // st 0: any plane of the chunk (every test on the chunk position at run time).  st 1: a
  // steady-state plane, kb + 2 <= mm <= mlast - 2 (the range is derived at the z-loop below), of a
  // launch without u_noise (a.noise null, as in every run with u_noise_amp == 0): each of those
  // tests is decided and compiled out, so the phases are straight-line code but for the per-lane
  // predicates isA, isB and is_x.  The arithmetic is the same text.
  auto step = [&](auto ph, auto st, int mm, PairRaw& rc, PairRaw& rn, PairRaw& rnn) -> bool {
    constexpr int PH = decltype(ph)::value;
    constexpr int ST = decltype(st)::value;
    constexpr bool SDY = ST != 0;
    constexpr int sA = PH, sAm = (PH + 2) % 3, sAp = (PH + 1) % 3;   // ring slots of planes mm, mm-1, mm+1
#if defined(__HIP_DEVICE_COMPILE__)
    // (the steady loop's plane index is laundered like the kernarg pointer: seen as an induction
    // variable, the plane offsets became a running per-lane offset and six products kept across
    // the loop, and pair 4+5 spilled the VGPRs the general steps need around the loop)
    if (SDY) asm volatile("" : "+s"(mm));
#endif
    {
      PFT_PAIR_BIND(A0, C0);
      (void)C0;
      if (GLB) glm = ZREG ? IA[sAp][2] : LD::ld(lA[sAp][2], posA);   // plane mm - 2, before mm + 1 replaces it
      // stage A's input of plane mm + 1 (own pair: read back by this thread in this iteration;
      // x/y neighbours: in the next one, behind the barrier), and the look-ahead load of plane
      // mm + 2.  Both unconditional -- beyond mlast the load re-reads plane mlast and the store
      // lands in the ring slot of plane mm - 2, which nobody reads any more -- so that no branch
      // separates a load from its use: with the loads under a branch the compiler's s_waitcnt
      // placement lost track of them and stage A waited for the look-ahead it had just issued.
      if (SDY || mm + 1 <= mlast) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const dbl2 v = pair_in_A<SA, GLX>(A0, q, rn);
          LD::st(lA[sAp][q], posA, v);
          if (ZREG) IA[sAp][q] = v;
        }
      }
      // The extra positions (last wave only, the test on wid is wave-uniform).  Plane mm + 1's
      // operands are in rc, loaded a step ago (the prologue's into R[0]): their stage-A input goes
      // into lA here, beside the own position's, ahead of the barrier.  Then plane mm + 2's operands
      // into rn, which a load-only lane is done with: its next readers, as rc, are the next step's
      // stage-B input and lO store, on rows it does not hold.  The loads go out ahead of the own
      // position's look-ahead: loads count in issue order, so the wait for that look-ahead at the
      // top of the next step covers these too, and the other waves, which skip the branch, wait for
      // theirs exactly as without it.  (Behind the look-ahead, the compiler's count for it would
      // have to assume these in flight after it in every wave, and drain to zero.)  Every load has
      // its consumer: mm + 2 <= mlast <= ke + 1 leaves mm < ke, so the next step runs.  The last
      // wave holds no stage-B position (pair_pos), so its SIMD has the wave-phase to spare.
      if constexpr (LWP == 22) {
        if (is_x(A0)) {
          if (SDY || mm + 1 <= mlast) xstore(A0, sAp, rc);
          if (SDY || mm + 2 <= mlast) xload(A0, mm + 2, rn);
        }
      }
      if (SDY || mm + 2 <= mlast) pair_load<SA>(A0, pbo(mm + 2), rnn);   // look-ahead
    }
    const int kB = mm - 1;                                   // stage B's plane
    constexpr int sB = (PH + 2) % 3, sBm = (PH + 1) % 3, sBp = PH;   // slots of planes kB, kB-1, kB+1
    // (GLB: gl's plane from lA, whose rows start one row earlier: slot posB + LWP there)
    const double* lBgl = GLB ? &lA[sB][2][2 * LWP] : &lB[sB][NBQ - 1][0];
    PairRaw ro;
    PairNbr hn;
    {
      PFT_PAIR_BIND(A1, C1);
      // The two waves of a SIMD (w and w + 4) run the same phase between two barriers, so their
      // stalls coincide.  Waves 0-3 get issue precedence in stage A (pair 2+3: waves 4-7 in stage
      // B, pair 4+5: nobody), so the two drift apart and fill each other's stalls.  Measured (A/B,
      // one box): pair 4+5 0.496 -> 0.480 ms; pair 2+3 0.425 -> 0.403 ms.
      if (PRIOF) {
        if ((threadIdx.x >> 8) == 0) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(0);
      }
      dbl2 (&ka)[2] = KA[PH];
      ka[0] = ka[1] = zero2;
      if ((SDY || mm <= mA1) && isA) {
        // stage A at plane mm, evaluated as the acting pair's thread does
        if (!SDY && mm == n3 - 1 && whi) {
          // top wall: the ring slot of plane n3 holds the ghost values -- Dirichlet u (equation.c:
          // 175-183), p and gl mirrored -- at this position (its own z neighbour only)
#pragma unroll
          for (int q = 1; q < 3; ++q) LD::st(lA[sAp][q], posA, LD::ld(lA[sA][q], posA));
          LD::st(lA[sAp][0], posA, dbl2{A1.T_topA, A1.T_topA});
          if (ZREG) {
            IA[sAp][1] = IA[sA][1];
            IA[sAp][2] = IA[sA][2];
            IA[sAp][0] = dbl2{A1.T_topA, A1.T_topA};
          }
        }
        dbl2 zc[3], zm[3], zp[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          zc[q] = ZREG ? IA[sA][q] : LD::ld(lA[sA][q], posA);
          zm[q] = ZREG ? IA[sAm][q] : LD::ld(lA[sAm][q], posA);
          zp[q] = ZREG ? IA[sAp][q] : LD::ld(lA[sAp][q], posA);
        }
        double du[2], dp[2];
        const double* nz = SDY ? nullptr : A1.noise ? A1.noise + (long)mm * A1.plane + (long)apo : nullptr;
        pair_rhs<MODE, LWP>(C1, lA[sA][0], lA[sA][1], lA[sA][2], actA, xmcA, xpcA, zm, zc, zp, nz, fzA, du, dp);
        ka[0] = dbl2{du[0], du[1]};
        ka[1] = dbl2{dp[0], dp[1]};
#pragma unroll
        for (int q = 0; q < NBQ; ++q) {
          const dbl2 ib = pair_in_B<SA, GLX>(A1, q, rc, q < 2 ? ka[q < 2 ? q : 0] : zero2);
          LD::st(lB[sA][q], posB, ib);
          if (!SDY && mm == 0 && wlo) LD::st(lB[sAm][q], posB, ib);   // bottom wall: plane -1 mirrors plane 0
        }
      }
    }
    if constexpr (STG) {
      // The stagger: the late half passes this step's barrier here, between stage A and stage B
      // (the early half at the step's end), so its stage B runs beside the early half's top and
      // stage A of the next step.  The top of that step overwrites lA's slot sB, whose field 2
      // stage B reads at its x/y neighbours (GLB): both halves read those six doubles here, where
      // the slot is intact, and the barrier's lgkmcnt(0) completes them.  The chunk's last step
      // has no barrier in either half.  (The hazard table is beside the z-loop.)
      if (GLB && (SDY || kB >= kb) && isB) hn = pair_nbr2<LWP>(lBgl, posB, xmcB, xpcB);
      if (late && (SDY || mm != ke)) __syncthreads();
    }
    {
      PFT_PAIR_BIND(A2, C2);
      if (PRIOF) {
        if (SA == 4) __builtin_amdgcn_s_setprio(0);
        else if ((threadIdx.x >> 8) == 0) __builtin_amdgcn_s_setprio(0);
        else __builtin_amdgcn_s_setprio(2);
      }
      // operands of plane kB for stage B's outputs (4+5).  OPL: from lO.  Otherwise loaded a
      // second time, after stage A (in registers they would need ~60 VGPRs more than the 255 in
      // use), and NOT an L2 hit: their first load was the look-ahead three planes earlier, and
      // three planes of the ring's operands of the ~32 workgroups of an XCD (~5 MB) exceed its
      // 4 MB L2 -- the Infinity Cache serves them (PMC: 1.80x the algorithmic bytes beyond L2
      // with the re-load, 1.11x with lO; pair 4+5 -1.5%: DESIGN.md section 5)
      // (GLX: gl's x(t+h) is not stored, XN holds it: gl's x is not needed)
      // (unconditional, as the look-ahead: every lane's acting pair is in the domain)
      if (OPL) {
        // plane kB's operands from lO, then plane mm's into the same slot (this thread's own; LDS
        // accesses of a wave stay in order)
        if ((SDY || kB >= kb) && isB) {
          ro.x[0] = lO[0][ob];
          ro.x[1] = lO[1][ob];
          ro.k1[0] = lO[2][ob];
          ro.k1[1] = lO[3][ob];
          ro.k3[0] = lO[4][ob];
          ro.k3[1] = lO[5][ob];
        }
        if (isB && (SDY || (mm >= kb && mm < ke))) {
          lO[0][ob] = rc.x[0];
          lO[1][ob] = rc.x[1];
          lO[2][ob] = rc.k1[0];
          lO[3][ob] = rc.k1[1];
          lO[4][ob] = rc.k3[0];
          lO[5][ob] = rc.k3[1];
        }
      } else if (SA == 4 && (SDY || kB >= kb) && isB) {
        pair_load<SA, !GLX>(A2, pbo(kB), ro);
      }
      if ((SDY || kB >= kb) && isB) {
        const int lo = posB;
        if (!SDY && kB == n3 - 1 && whi) {
          // top wall: the ghost values of plane n3 at this position (as in stage A above)
#pragma unroll
          // (GLB: gl's ghost is in lA's slot of plane n3, from stage A's top wall)
          for (int q = 1; q < NBQ; ++q) LD::st(lB[sBp][q], lo, LD::ld(lB[sB][q], lo));
          LD::st(lB[sBp][0], lo, dbl2{A2.T_topB, A2.T_topB});
        }
        dbl2 zc[3], zm[3], zp[3];
#pragma unroll
        for (int q = 0; q < NBQ; ++q) {
          zc[q] = LD::ld(lB[sB][q], lo);
          zm[q] = LD::ld(lB[sBm][q], lo);
          zp[q] = LD::ld(lB[sBp][q], lo);
        }
        if (GLB) {
          zc[2] = ZREG ? IA[sB][2] : LD::ld(lA[sB][2], posA);
          zm[2] = glm;
          zp[2] = ZREG ? IA[sBp][2] : LD::ld(lA[sBp][2], posA);
        }
        if (!SDY && kB == kb) {
          // the z-face below the chunk's first stage-B plane
#pragma unroll
          for (int s = 0; s < 2; ++s)
            fzB[s] = face_of(C2, zm[1][s], zm[2][s], zm[0][s], zc[1][s], zc[2][s], zc[0][s], FLUX);
        }
        double du[2], dp[2];
        const unsigned e0 = pbo(kB);
        const double* nz = SDY ? nullptr : A2.noise ? A2.noise + (long)kB * A2.plane + (long)apo : nullptr;
        pair_rhs<MODE, LWP, STG && GLB>(C2, lB[sB][0], lB[sB][1], lBgl, lo, xmcB, xpcB, zm, zc, zp, nz, fzB, du, dp, &hn);
        if (SA == 2) {
          stb(A2.out, e0, dbl2{du[0], du[1]});                   // K3 (hybrid2.c:412-429)
          stb(A2.out + A2.fs, e0, dbl2{dp[0], dp[1]});
        } else {
          const dbl2(&kao)[2] = KA[(PH + 2) % 3];              // stage A's K (K4) at plane kB
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const dbl2 K = q == 0 ? dbl2{du[0], du[1]} : dbl2{dp[0], dp[1]};
            const dbl2 k1 = ro.k1[q], k3 = ro.k3[q], k4 = kao[q];
            const double em = q == 0 ? A2.em0 : A2.em1;
            dbl2 r;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
              const double ev = em * fabs(0.2 * k1[s] - 0.9 * k3[s] + 0.8 * k4[s] - 0.1 * K[s]);   // :521
              if (ev > m) m = ev;                                                            // NaN never wins
              nf |= !isfinite(ev);
              r[s] = ro.x[q][s] + A2.coef * (0.5 * (k1[s] + K[s]) + 2.0 * k4[s]);            // :667
            }
            stb(A2.out + q * A2.fs, e0, r);
          }
          // gl: x(t+h) = x + coef (0.5 (0.0 + 0.0) + 2.0 0.0), stored unless XN already holds it
          if (!GLX && !A2.gl_keep) stb(A2.out + 2 * A2.fs, e0, dbl2{ro.x[2][0] + A2.glX, ro.x[2][1] + A2.glX});
        }
      }
    }
    if (!SDY && mm == ke) return false;
    if (!STG || !late) __syncthreads();
    return true;
  };

  // The staggered schedule and its LDS accesses (STG; tests/test_pair_stagger_model.py restates
  // this table and checks it).  Step j runs T_j (the top), A_j (stage A, plane j), B_j (stage B,
  // plane j - 1); bar_j is its barrier and interval I_j lies between bar_{j-1} and bar_j.  The
  // early half runs T_j A_j B_j bar_j, the late half T_j A_j bar_j B_j: the early half's I_j holds
  // T_j A_j B_j, the late half's B_{j-1} T_j A_j.  Both skip bar_j on the chunk's last step, so
  // every wave passes the prologue's barrier, one per step but the last, and the epilogue's: the
  // same count on every path (an empty chunk: none but the epilogue's).  slot(p) = (p - mA0) mod 3.
  //
  //   access                      ring slot, fields     position    interval: early / late
  //   T_j   glm read (4+5, GLB)   lA slot(j+1), 2       own         I_j / I_j
  //   T_j   plane j+1 in          lA slot(j+1), 0-2     own, extras I_j / I_j
  //   A_j   top wall ghost        lA slot(j+1), 0-2     own         I_j / I_j   (T_j stores nothing there)
  //   A_j   x/y neighbours        lA slot(j), 0-2       neighbours  I_j / I_j   (actA's: the same reads)
  //   A_j   z column (4+5)        lA slot(j-1 .. j+1)   own         I_j / I_j
  //   A_j   stage B's input out   lB slot(j), 0-NBQ     own         I_j / I_j   (bottom wall: slot(j-1) too)
  //   hoist gl x/y neighbours     lA slot(j-1), 2       neighbours  I_j / I_j   (GLB; ahead of bar_j)
  //   B_j   top wall ghost        lB slot(j), 0-NBQ     own         I_j / I_j+1 (last step only: no I_j+1)
  //   B_j   x/y neighbours        lB slot(j-1), 0-NBQ   neighbours  I_j / I_j+1
  //   B_j   z column              lB slot(j-2 .. j)     own         I_j / I_j+1
  //   B_j   gl centre, above      lA slot(j-1), slot(j), 2  own     I_j / I_j+1 (GLB, 4+5; registers in 2+3)
  //   B_j   operands              lO                    own         I_j / I_j+1
  //
  // A neighbour read is safe when its slot and field are written in an earlier interval and not in
  // its own.  lA slot(j) is written in I_{j-1} (T_{j-1}) and again in I_{j+2}: A_j's reads in I_j
  // are safe in both halves.  lB slot(j-1) is written in I_{j-1} (A_{j-1}) and again in I_{j+2}
  // (A_{j+2}): B_j's reads in I_j or I_{j+1} are safe.  The early half's A_{j+1} writes lB
  // slot(j+1) = slot(j-2) while the late half's B_j reads that slot, but each at its own position.
  // The hazard is B_j's gl neighbours under GLB: lA slot(j-1) is overwritten by T_{j+1} in I_{j+1},
  // where the late half's B_j runs -- hence the hoist into I_j, where the writes go to slot(j+1)
  // (T_j and stage A's top wall).  Own-position accesses stay in program order, which is the same
  // in both halves.  (Threads beyond the positions shadow the last one: the same values into the
  // same slot in the same interval as its owner, T_j's row of the table.)
  if (kb < ke) {
    // The steady range.  A step at plane mm has every chunk-position test of step() decided when
    //   mm + 2 <= mlast   the look-ahead, the next plane's stage-A input and the extras' pair of
    //                     them all run; with mlast <= mA1 + 1 and mA1 <= ke this also gives
    //                     mm <= mA1 - 1 (stage A runs, not on a wall plane: at a top wall
    //                     mlast = n3 - 1, so mm <= n3 - 3), mm < ke (lO is written, the chunk
    //                     goes on) and kB = mm - 1 < n3 - 1 (no top wall in stage B);
    //   mm >= kb + 2      stage B runs on a plane above the chunk's first (kB > kb: fzB is
    //                     carried, lO holds plane kB), and mm >= 2 is no bottom wall plane.
    // A triple of steps (the register rotation's period, starting at mA0 + 3j in phase 0) is
    // steady when its first and last step are: mm >= kb + 2 and mm + 4 <= mlast.  mA0 <= kb, so
    // the chunk's first triple never is; a two-plane boundary chunk (ke = kb + 2, mlast <= kb + 3)
    // and every chunk of fewer than five planes has none.  The steady triples are a loop of
    // their own; where it ends, the general triple takes the chunk's last steps (one to five).
    // A launch with u_noise has no steady triple: a steady body with the noise loads beside the
    // one without made every instance spill, so its planes all take
    // the general body, as before.  So do those of pair 4+5 in calc_mode 0 without GLX (a launch
    // whose gl holds a -0.0 or a NaN), the one kernel that kept a spilled VGPR with the steady
    // loop: it stays the single z-loop it was.  The 12-pair pitch keeps the single loop too:
    // 200^3 (100 x 100 planes) ran 1.6% slower with the steady loop, outside the run-to-run range
    // (profiles/f9_bench_ab.txt).  The stagger (STG) is decided per instance as well, by
    // pair_stagger above the kernel: pair 2+3 on the 22-pair pitch in calc_modes 0 and 1 has it, general and
    // steady steps alike; pair 4+5 and the 12-pair pitch keep every wave's barrier at the step's end.
    constexpr bool STEADY = LWP == 22 && !(SA == 4 && MODE == 0 && !GLX);
    const int msteady = a.noise ? -(1 << 30) : mlast - 4;        // last first plane of a steady triple
    for (int mm = mA0;; mm += 3) {
      if (STEADY && mm >= kb + 2) {
        for (; mm <= msteady; mm += 3) {
          step(pft_ic<0>{}, pft_ic<1>{}, mm, R[0], R[1], R[2]);
          step(pft_ic<1>{}, pft_ic<1>{}, mm + 1, R[1], R[2], R[0]);
          step(pft_ic<2>{}, pft_ic<1>{}, mm + 2, R[2], R[0], R[1]);
        }
      }
      if (!step(pft_ic<0>{}, pft_ic<0>{}, mm, R[0], R[1], R[2])) break;
      if (!step(pft_ic<1>{}, pft_ic<0>{}, mm + 1, R[1], R[2], R[0])) break;
      if (!step(pft_ic<2>{}, pft_ic<0>{}, mm + 2, R[2], R[0], R[1])) break;
    }
  }

  if (SA == 4) {
    __shared__ double red[PFT_PBLOCK / 64];
    __shared__ int rnf[PFT_PBLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(m, off, 64);
      if (ov > m) m = ov;
    }
    const int anynf = __any(nf);
    // (the wave and the lane as in the z-loop: threadIdx.x is not kept across it for these tests)
    const int w = wid;
    if (lane() == 0) {
      red[w] = m;
      rnf[w] = anynf;
    }
    __syncthreads();
    if (wid == 0 && lane() == 0) {
      double bm = red[0];
      int bnf = rnf[0];
      for (int q = 1; q < PFT_PBLOCK / 64; ++q) {
        if (red[q] > bm) bm = red[q];
        bnf |= rnf[q];
      }
      // (the norm's arguments re-read here like the z-loop's: loaded with the prologue's, the
      // compiler carried these twelve SGPRs across the whole kernel in spill lanes)
      PFT_PAIR_BIND(AE, CE);
      (void)CE;
      // gl's error-norm term: the same constant at every cell (its K's are literal zeros)
      if (AE.evgl > bm) bm = AE.evgl;
      bnf |= !isfinite(AE.evgl);
      if (AE.part) eps_store_part(AE.part, bm, bnf);
      else eps_arrive(bm, bnf, AE.shards, AE.eps_bits, AE.nonfinite, AE.pub, AE.pub_count);
    }
  }
  if (bw) {
    // an inline boundary workgroup: every wave's stores done, then one lane writes the XCD's L2
    // back (system scope: the copy engines read memory, not this L2) and counts the workgroup; the
    // copies wait for the count (bnd_trigger_kernel) while the interior workgroups go on
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wid == 0 && lane() == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      __hip_atomic_fetch_add(a.bdone, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
#pragma clang diagnostic pop

// ------------------------------------------------------------------------------------------
// layout conversion kernels (host padded layout, ghost thickness 2 <-> device layout)

__global__ void publish_kernel(unsigned long long* __restrict__ d, unsigned long long* host)
{
  host[0] = d[0];
  host[1] = d[1];
  d[0] = 0;              // ready for the next step's error norm (no separate fill)
  d[1] = 0;
  __threadfence_system();
}

__global__ void pack_kernel(const double* __restrict__ host, double* __restrict__ dev, int n1, int n2,
                            int n3, long fs, long S)
{
  // planes -1..n3 of every field (ghost planes included)
  const long plane = (long)n1 * n2;
  const long total = 3L * (n3 + 2) * plane;
  const int N1 = n1 + 4, N2 = n2 + 4;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int q = (int)(e / ((n3 + 2) * plane));
    const long r = e - (long)q * (n3 + 2) * plane;
    const int kk = (int)(r / plane);          // 0..n3+1 = k+1
    const long c = r - (long)kk * plane;
    const int j = (int)(c / n1), i = (int)(c - (long)j * n1);
    dev[q * fs + r] = host[q * S + (long)(kk + 1) * N1 * N2 + (long)(j + 2) * N1 + (i + 2)];
  }
}

__global__ void unpack_kernel(const double* __restrict__ dev, double* __restrict__ host, int n1, int n2,
                              int n3, long fs, long S)
{
  // interior planes only
  const long plane = (long)n1 * n2;
  const long total = 3L * n3 * plane;
  const int N1 = n1 + 4, N2 = n2 + 4;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int q = (int)(e / (n3 * plane));
    const long r = e - (long)q * n3 * plane;
    const int k = (int)(r / plane);
    const long c = r - (long)k * plane;
    const int j = (int)(c / n1), i = (int)(c - (long)j * n1);
    host[q * S + (long)(k + 2) * N1 * N2 + (long)(j + 2) * N1 + (i + 2)] = dev[q * fs + (long)(k + 1) * plane + c];
  }
}

// ------------------------------------------------------------------------------------------
// generic chunk-table combines (host-staged path for unregistered right-hand sides)

__global__ void flat_combine_kernel(int stage, int n_chunks, const int* __restrict__ cstart,
                                    const int* __restrict__ csize, const double* __restrict__ cmult,
                                    double coef, double h, const double* x, const double* k1,
                                    const double* k2, const double* k3, const double* k4,
                                    const double* k5, double* out, unsigned long long* eps_bits,
                                    unsigned int* nonfinite)
{
  double m = 0.0;
  bool nf = false;
  for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const long s0 = cstart[ch];
    const int n = csize[ch];
    const double mult = cmult ? cmult[ch] : 1.0;
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
      const long e = s0 + t;
      switch (stage) {
        case 1: out[e] = k1[e] * coef + x[e]; break;                              // :388
        case 2: out[e] = (k1[e] + k2[e]) * coef + x[e]; break;                    // :408
        case 3: out[e] = (k1[e] + 3.0 * k3[e]) * coef + x[e]; break;              // :428
        case 4: out[e] = (0.5 * k1[e] - 1.5 * k3[e] + 2.0 * k4[e]) * h + x[e]; break;  // :449
        case 5: {
          const double ev = mult * fabs(0.2 * k1[e] - 0.9 * k3[e] + 0.8 * k4[e] - 0.1 * k5[e]);
          if (ev > m) m = ev;
          nf |= !isfinite(ev);
        } break;
        case 6: out[e] += coef * (0.5 * (k1[e] + k5[e]) + 2.0 * k4[e]); break;    // :667
      }
    }
  }
  if (stage == 5) {
    __shared__ double red[PFT_BLOCK / 64];
    __shared__ int rnf[PFT_BLOCK / 64];
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(m, off, 64);
      if (o > m) m = o;
    }
    const int anynf = __any(nf);
    if ((threadIdx.x & 63) == 0) {
      red[threadIdx.x >> 6] = m;
      rnf[threadIdx.x >> 6] = anynf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double bm = red[0];
      int bnf = rnf[0];
      for (int k = 1; k < (int)(blockDim.x / 64); ++k) {
        if (red[k] > bm) bm = red[k];
        bnf |= rnf[k];
      }
      if (bm > 0.0) atomicMax(eps_bits, (unsigned long long)__double_as_longlong(bm));
      if (bnf) atomicOr(nonfinite, 1u);
    }
  }
}

// ------------------------------------------------------------------------------------------
// calibration probe: a plain 8-byte-per-lane copy with a known byte count, used to calibrate
// rocprofv3's FETCH_SIZE / WRITE_SIZE for the access width the stage kernels use

__global__ void probe_copy_kernel(double* __restrict__ dst, const double* __restrict__ src, long n)
{
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x)
    dst[e] = src[e];
}

// ------------------------------------------------------------------------------------------
// slab object + shim

static double wall_s()
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec + 1e-9 * t.tv_nsec;
}

// A dead or diverged ipc peer never raises the flag word the compute stream waits on
// (hipStreamWaitValue64, pft_slab_halo_wait), so the stream would never drain.  On expiry of
// s->timeout_s the slab raises its own flag words past every sequence number (on the side stream,
// which nothing blocks): the compute stream drains -- its results are void -- and the caller gets
// PFT_ERR_IPC_TIMEOUT, which RK_MPI_SA_solve reports as PFT_SOLVE_DEVICE_ERROR.
int slab_poisoned(pft_slab* s, const char* what)
{
  if (s->ipc_poisoned == 2) {
    snprintf(g_err, sizeof(g_err), "%s: the slab's communicator was aborted (PFT_COMM_TIMEOUT or an asynchronous error)", what);
    return PFT_ERR_COMM_ABORTED;
  }
  snprintf(g_err, sizeof(g_err), "%s: an earlier ipc halo wait timed out; detach and re-attach the slab", what);
  return PFT_ERR_IPC_TIMEOUT;
}

// the communicator watchdog (pft_slab_set_watch), called about every millisecond of a host wait;
// t0: when the wait began (0: not yet taken).  Nonzero: the communicator aborted -- the slab
// refuses from now on (its streams drained inside the abort, or will never: no later wait trusts them)
static int slab_watch(pft_slab* s, double* t0, const char* what)
{
  if (*t0 == 0.0) *t0 = wall_s();
  const int expired = wall_s() - *t0 > s->watch_timeout_s;
  const int rc = s->watch(s->watch_ctx, expired);
  if (!rc) return 0;
  s->ipc_poisoned = 2;
  snprintf(g_err, sizeof(g_err), "%s: the communicator aborted (%s)", what,
           expired ? "no progress within PFT_COMM_TIMEOUT" : "asynchronous error");
  fprintf(stderr, "libpft: %s\n", g_err);
  return rc;
}

static int slab_timed_out(pft_slab* s, const char* what)
{
  static const unsigned long long released[2] = {~0ULL >> 1, ~0ULL >> 1};
  s->ipc_poisoned = 1;
  // on a stream of its own: the slab's other streams may hold copies waiting (through events) for
  // the blocked compute stream (the copy-engine exchange)
  hipStream_t rel = nullptr;
  if (hipStreamCreateWithFlags(&rel, hipStreamNonBlocking) == hipSuccess) {
    (void)hipMemcpyAsync(s->sig, released, sizeof(released), hipMemcpyHostToDevice, rel);
    (void)hipStreamSynchronize(rel);
    (void)hipStreamDestroy(rel);
  }
  (void)hipStreamSynchronize(s->stream);
  (void)hipGetLastError();
  snprintf(g_err, sizeof(g_err), "%s: no halo from an ipc neighbour within %.0f s (PFT_IPC_TIMEOUT)", what,
           s->timeout_s);
  fprintf(stderr, "libpft: %s\n", g_err);
  return PFT_ERR_IPC_TIMEOUT;
}

// the host waits for an event (or the whole compute stream when ev is null): unbounded with no ipc
// peer, bounded by s->timeout_s with one
int slab_wait(pft_slab* s, hipEvent_t ev, const char* what)
{
  if (s->ipc_poisoned) {
    // ipc: the released flags let the stream drain: wait for it, then refuse.  An aborted
    // communicator: refuse at once (nothing guarantees the stream drains)
    if (s->ipc_poisoned == 1) (void)hipStreamSynchronize(s->stream);
    (void)hipGetLastError();
    return slab_poisoned(s, what);
  }
  if (!ev && s->bnd_mode == 3 && s->bnd && s->ev_join) {
    // the boundary pipeline: a wait for the compute stream includes the boundary stream (its
    // halo waits and staged receives write ghost planes the host or the next call may read)
    HIPCHK(hipEventRecord(s->ev_join, s->bnd));
    HIPCHK(hipStreamWaitEvent(s->stream, s->ev_join, 0));
  }
  if (!s->peer[0].on && !s->peer[1].on && !s->watch) {
    HIPCHK(ev ? hipEventSynchronize(ev) : hipStreamSynchronize(s->stream));
    return 0;
  }
  const double t0 = wall_s();
  double tw = 0.0;
  for (long it = 0;; ++it) {
    const hipError_t q = ev ? hipEventQuery(ev) : hipStreamQuery(s->stream);
    if (q == hipSuccess) return 0;
    if (q != hipErrorNotReady) return fail(q, what);
    if (it < 20000) {
      __builtin_ia32_pause();
    } else {
      sched_yield();
      if ((it & 1023) == 0) {
        if (s->watch) {
          const int rc = slab_watch(s, &tw, what);
          if (rc) return rc;
        } else if (wall_s() - t0 > s->timeout_s) {
          return slab_timed_out(s, what);
        }
      }
    }
  }
}

extern "C" {

int pft_slab_sync(pft_slab* s) { return s ? slab_wait(s, nullptr, "pft_slab_sync") : -2; }

int pft_slab_set_watch(pft_slab* s, pft_slab_watch_fn fn, void* ctx, double timeout_s)
{
  if (!s || (fn && !(timeout_s > 0.0))) return -2;
  s->watch = fn;
  s->watch_ctx = fn ? ctx : nullptr;
  s->watch_timeout_s = timeout_s;
  return 0;
}

const char* pft_hip_last_error(void) { return g_err; }

int pft_hip_device_count(int* n)
{
  HIPCHK(hipGetDeviceCount(n));
  return 0;
}
int pft_hip_set_device(int dev)
{
  HIPCHK(hipSetDevice(dev));
  return 0;
}
int pft_hip_get_device(int* dev)
{
  HIPCHK(hipGetDevice(dev));
  return 0;
}

int pft_hip_device_phys_id(int dev, int* id)
{
  // the GPU's PCI location (domain, bus, device): the same physical GPU has the same id in every
  // process, whatever each process's device numbering (HIP_VISIBLE_DEVICES)
  int dom = 0, bus = 0, pdev = 0;
  HIPCHK(hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainId, dev));
  HIPCHK(hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, dev));
  HIPCHK(hipDeviceGetAttribute(&pdev, hipDeviceAttributePciDeviceId, dev));
  *id = ((dom & 0xffff) << 13) | ((bus & 0xff) << 5) | (pdev & 0x1f);
  return 0;
}
int pft_hip_device_ident(int dev, char* buf, int len)
{
  if (!buf || len < PFT_DEV_IDENT_BYTES) return -2;
  char bus[32] = {0};
  hipUUID u;
  memset(&u, 0, sizeof(u));
  HIPCHK(hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, dev));
  HIPCHK(hipDeviceGetUuid(&u, dev));
  int n = snprintf(buf, (size_t)len, "%s/", bus);
  for (int i = 0; i < 16 && n < len - 2; ++i) n += snprintf(buf + n, (size_t)(len - n), "%02x", (unsigned char)u.bytes[i]);
  return 0;
}
int pft_hip_device_sync(void)
{
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

static long pair_geometry(int n1, int n2, int* tx_out, int* ty_out);

// c.ralpha for s->c.alpha (div_alpha): one lane on the device, when alpha changes
static int slab_div_consts(pft_slab* s)
{
  if (!s->da_valid || memcmp(&s->da_alpha, &s->c.alpha, sizeof(double)) != 0) {
    double* d = nullptr;
    double h = 0.0;
    hipError_t e = hipMalloc((void**)&d, sizeof(h));
    if (e == hipSuccess) {
      div_alpha_consts_kernel<<<1, 1, 0, s->stream>>>(s->c.alpha, d);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (d) (void)hipFree(d);
    if (e != hipSuccess) return fail(e, "div_alpha constants");
    s->da_alpha = s->c.alpha;
    s->da_r = h;
    s->da_valid = 1;
  }
  s->c.ralpha = s->da_r;
  return 0;
}

int pft_slab_create(pft_slab** out, const pft_slab_desc* d, const pft_consts* c)
{
  *out = nullptr;
  if (d->n1 < 1 || d->n2 < 1 || d->n3 < 1) return -2;
  pft_slab* s = new pft_slab();
  memset(s, 0, sizeof(*s));
  s->d = *d;
  s->c = *c;
  s->plane = d->n1 * d->n2;
  // a field: far ghost plane, ghost plane, n3 interior planes, ghost plane, far ghost plane; the
  // buffer pointer points at the first ghost plane (plane 0 of the kernels' indexing)
  const long raw = (long)(d->n3 + 4) * s->plane;
  s->fs = (raw + 63) & ~63L;  // 512-byte aligned field strides
  s->S = (long)(d->n1 + 4) * (d->n2 + 4) * (d->n3 + 4);
  s->kz = 0;
  s->tile_wx = 1;
  s->n1_tiled_ok = 1;
  s->recompute = 1;
  {
    // fault injection (tests/test_ipc_multiprocess.py): this slab never delivers its halo -- no
    // put, no flag raise -- as a peer that died would not
    const char* ed = getenv("PFT_IPC_DROP_PUTS");
    s->drop_puts = ed ? atoi(ed) : 0;
    // pair kernels where the slab qualifies (pft_slab_pair_ok); env PFT_PAIR=0 turns them off (A/B)
    const char* ep = getenv("PFT_PAIR");
    s->pair_env = ep != nullptr;
    s->pair_on = ep ? atoi(ep) : 1;
    s->pair_ntile = pair_geometry(d->n1, d->n2, &s->pair_tx, &s->pair_ty);
    const char* eg = getenv("PFT_GATE_FLIP");
    s->gate_flip = eg ? atoi(eg) : 0;
    const char* ew = getenv("PFT_WAIT_STREAMOPS");
    s->wait_streamops = ew ? atoi(ew) : 0;
    const char* et = getenv("PFT_IPC_TIMEOUT");
    s->timeout_s = (et && atof(et) > 0.0) ? atof(et) : 300.0;
    const char* edg = getenv("PFT_DIAG_WGS");
    s->diag_wgs = (edg && atoi(edg) > 0) ? atoi(edg) : 0;
    const char* erg = getenv("PFT_REGION_WGS");
    s->region_wgs = (erg && atoi(erg) > 0) ? atoi(erg) : 0;
  }
  const size_t bytes = sizeof(double) * (3 * (size_t)s->fs + 2 * (size_t)s->plane);
  hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
  // the halo exchange's stream at the greatest priority: its RCCL kernel is dispatched ahead of
  // the interior sweep's workgroups when both become ready
  int prio_lo = 0, prio_hi = 0;
  if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&s->comm, hipStreamNonBlocking, prio_hi);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_eps, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_order[0], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_order[1], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_order[2], hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc((void**)&s->scratch, 64);
  if (e == hipSuccess) e = hipHostMalloc((void**)&s->host_scratch, 64, hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void**)&s->host_pub, 64, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&s->host_pub_dev, s->host_pub, 0);
  if (e == hipSuccess)
    e = hipHostMalloc((void**)&s->pub_ring, 16 * PFT_PUB_SLOTS, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&s->pub_ring_dev, s->pub_ring, 0);
  if (e == hipSuccess)
    e = hipHostMalloc((void**)&s->gate_pin, 32 * PFT_GATE_SLOTS, hipHostMallocMapped | hipHostMallocCoherent);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&s->gate_pin_dev, s->gate_pin, 0);
  if (e == hipSuccess) memset(s->gate_pin, 0, 32 * PFT_GATE_SLOTS);
  if (e == hipSuccess) e = hipMalloc((void**)&s->gate_dev, 32 * PFT_GATE_SLOTS);
  if (e == hipSuccess) e = hipMemsetAsync(s->gate_dev, 0, 32 * PFT_GATE_SLOTS, s->stream);
  // two sets of error-norm shards: a boundary launch uses the second, so that it may run beside the
  // interior launch of the same stage (pft_slab_set_boundary_stream)
  const size_t cnt_bytes = 64 + sizeof(EpsShard) * 2 * PFT_EPS_SHARDS;
  if (e == hipSuccess) e = hipMalloc((void**)&s->pub_count, cnt_bytes);
  if (e == hipSuccess) e = hipMemsetAsync(s->pub_count, 0, cnt_bytes, s->stream);
  if (e == hipSuccess) s->eps_shards = (EpsShard*)((char*)s->pub_count + 64);
  // the flag words are polled by the command processor (hipStreamWaitValue64) and written by a
  // neighbour -- possibly another GPU over xGMI: uncached device memory, so that no cache between
  // the writer and the poller can hold a stale copy
  if (e == hipSuccess) e = hipExtMallocWithFlags((void**)&s->sig, 4096, hipDeviceMallocUncached);
  if (e == hipSuccess) e = hipMemsetAsync(s->sig, 0, 4096, s->stream);
  for (int b = 0; b < PFT_BUF_COUNT && e == hipSuccess; ++b) {
    e = hipMalloc((void**)&s->buf0[b], bytes);
    s->buf[b] = s->buf0[b] + s->plane;   // past the first field's far ghost plane
    s->phys[b] = b;
    // zero-fill on the slab's own stream: the compute stream is non-blocking, so a fill on the
    // null stream would not be ordered before the first upload/kernel (it raced with them)
    if (e == hipSuccess) e = hipMemsetAsync(s->buf0[b], 0, bytes, s->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  int dev = 0;
  if (e == hipSuccess) e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&s->n_cu, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) {
    pft_slab_destroy(s);
    return fail(e, "slab buffers/streams");
  }
  if (int rc = slab_div_consts(s)) {
    pft_slab_destroy(s);
    return rc;
  }
  *out = s;
  return 0;
}

int pft_slab_destroy(pft_slab* s)
{
  if (!s) return 0;
  (void)pft_slab_ipc_close(s);
  for (int b = 0; b < PFT_BUF_COUNT; ++b)
    if (s->buf0[b]) (void)hipFree(s->buf0[b]);
  if (s->sig) (void)hipFree(s->sig);
  if (s->rbuf) (void)hipFree(s->rbuf);
  if (s->seqtab) (void)hipFree(s->seqtab);
  if (s->seqhost) (void)hipHostFree(s->seqhost);
  if (s->staging) (void)hipFree(s->staging);
  if (s->noise) (void)hipFree(s->noise);
  for (int st = 0; st < 6; ++st)
    for (int e = 0; e < 2; ++e)
      for (int r = 0; r < PFT_TRING; ++r)
        if (s->tev[st][r][e]) (void)hipEventDestroy(s->tev[st][r][e]);
  if (s->diag_dev) (void)hipFree(s->diag_dev);
  if (s->diag_host) (void)hipHostFree(s->diag_host);
  for (int i = 0; i < 2; ++i)
    if (s->ev_diag[i]) (void)hipEventDestroy(s->ev_diag[i]);
  if (s->means_dev) (void)hipFree(s->means_dev);
  if (s->means_host) (void)hipHostFree(s->means_host);
  for (int i = 0; i < 2; ++i)
    if (s->ev_means[i]) (void)hipEventDestroy(s->ev_means[i]);
  if (s->formula_dev) (void)hipFree(s->formula_dev);
  if (s->formula_host) (void)hipHostFree(s->formula_host);
  if (s->formula_prog_dev) (void)hipFree(s->formula_prog_dev);
  if (s->formula_prog_host) (void)hipHostFree(s->formula_prog_host);
  for (int i = 0; i < 2; ++i)
    if (s->ev_formula[i]) (void)hipEventDestroy(s->ev_formula[i]);
  if (s->hist_dev) (void)hipFree(s->hist_dev);
  if (s->hist_host) (void)hipHostFree(s->hist_host);
  for (int i = 0; i < 2; ++i)
    if (s->ev_hist[i]) (void)hipEventDestroy(s->ev_hist[i]);
  if (s->map_dev) (void)hipFree(s->map_dev);
  if (s->map_host) (void)hipHostFree(s->map_host);
  for (int i = 0; i < 2; ++i)
    if (s->ev_map[i]) (void)hipEventDestroy(s->ev_map[i]);
  if (s->snap_host) {
    // the background writer may still read the image: it finishes first
    (void)pft_snapshot_writer_release(s->snap_host);
    (void)hipHostFree(s->snap_host);
  }
  if (s->snap_stage) (void)hipFree(s->snap_stage);
  for (int i = 0; i < 2; ++i)
    if (s->ev_snap[i]) (void)hipEventDestroy(s->ev_snap[i]);
  if (s->scratch) (void)hipFree(s->scratch);
  if (s->host_scratch) (void)hipHostFree(s->host_scratch);
  if (s->host_pub) (void)hipHostFree(s->host_pub);
  if (s->pub_ring) (void)hipHostFree(s->pub_ring);
  if (s->gate_pin) (void)hipHostFree(s->gate_pin);
  if (s->gate_dev) (void)hipFree(s->gate_dev);
  if (s->pub_count) (void)hipFree(s->pub_count);
  if (s->part) (void)hipFree(s->part);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  if (s->comm) (void)hipStreamDestroy(s->comm);
  if (s->side) (void)hipStreamDestroy(s->side);
  if (s->bnd) (void)hipStreamDestroy(s->bnd);
  if (s->ev_bnd) (void)hipEventDestroy(s->ev_bnd);
  if (s->ev_pre) (void)hipEventDestroy(s->ev_pre);
  if (s->ev_copy) (void)hipEventDestroy(s->ev_copy);
  if (s->ev_side) (void)hipEventDestroy(s->ev_side);
  if (s->ev_join) (void)hipEventDestroy(s->ev_join);
  if (s->ev_trig) (void)hipEventDestroy(s->ev_trig);
  if (s->bdone) (void)hipFree(s->bdone);
  for (int i = 0; i < 2; ++i) {
    if (s->ev_seq[i]) (void)hipEventDestroy(s->ev_seq[i]);
    if (s->ev_planes[i]) (void)hipEventDestroy(s->ev_planes[i]);
  }

  if (s->ev_eps) (void)hipEventDestroy(s->ev_eps);
  for (int i = 0; i < 3; ++i)
    if (s->ev_order[i]) (void)hipEventDestroy(s->ev_order[i]);
  delete s;
  return 0;
}

size_t pft_slab_state_bytes(const pft_slab* s) { return sizeof(double) * 3 * (size_t)s->fs; }
void* pft_slab_stream(pft_slab* s) { return (void*)s->stream; }
void* pft_slab_comm_stream(pft_slab* s) { return (void*)s->comm; }
double* pft_slab_buffer(pft_slab* s, int which) { return (which >= 0 && which < PFT_BUF_COUNT) ? s->buf[which] : nullptr; }
size_t pft_slab_field_stride(const pft_slab* s) { return (size_t)s->fs; }
size_t pft_slab_plane(const pft_slab* s) { return (size_t)s->plane; }
int pft_slab_nz(const pft_slab* s) { return s->d.n3; }
void* pft_slab_scratch(pft_slab* s) { return (void*)s->scratch; }
const pft_slab_desc* pft_slab_get_desc(const pft_slab* s) { return &s->d; }
int pft_slab_set_tile(pft_slab* s, int wx)
{
  if (wx != 0 && wx != 1 && wx != 2 && wx != 16 && wx != 32) return -2;
  s->tile_wx = wx;
  return 0;
}

int pft_slab_set_kz(pft_slab* s, int kz)
{
  if (kz < 0) return -2;
  s->kz = kz;
  return 0;
}

static int ensure_staging(pft_slab* s)
{
  if (s->staging) return 0;
  HIPCHK(hipMalloc((void**)&s->staging, sizeof(double) * 3 * (size_t)s->S));
  return 0;
}

int pft_slab_upload_host(pft_slab* s, int which, const double* host_padded)
{
  // X and XN may differ now: the caller re-establishes it (an upload of a stage buffer, e.g. A0
  // for a host-side RHS evaluation, leaves it alone)
  if (which == PFT_BUF_X || which == PFT_BUF_XN) s->gl_keep = 0;
  int rc = ensure_staging(s);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(s->staging, host_padded, sizeof(double) * 3 * (size_t)s->S, hipMemcpyHostToDevice,
                        s->stream));
  pack_kernel<<<2048, 256, 0, s->stream>>>(s->staging, s->buf[which], s->d.n1, s->d.n2, s->d.n3, s->fs, s->S);
  HIPCHK(hipGetLastError());
  return slab_wait(s, nullptr, "upload");
}

int pft_slab_download_host(pft_slab* s, int which, double* host_padded)
{
  int rc = ensure_staging(s);
  if (rc) return rc;
  // staging keeps the host's ghost values (copied in first), interior overwritten
  HIPCHK(hipMemcpyAsync(s->staging, host_padded, sizeof(double) * 3 * (size_t)s->S, hipMemcpyHostToDevice,
                        s->stream));
  unpack_kernel<<<2048, 256, 0, s->stream>>>(s->buf[which], s->staging, s->d.n1, s->d.n2, s->d.n3, s->fs, s->S);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(host_padded, s->staging, sizeof(double) * 3 * (size_t)s->S, hipMemcpyDeviceToHost,
                        s->stream));
  return slab_wait(s, nullptr, "download");
}

}  // extern "C"

// resident workgroups per CU of the kernel launch_stage would run (hipOccupancy..., cached)
template <int STAGE, int MODE, bool GLS>
static int kernel_occupancy(int kind)
{
  static int cache[2] = {0, 0};
  int& n = cache[kind == KFUSED];
  if (n) return n;
  const void* f = kind == KFUSED ? (const void*)merson_fused<STAGE, MODE, GLS>
                                 : (const void*)merson_stage<STAGE, MODE, GLS>;
  int b = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, f, kind == KFUSED ? PFT_FBLOCK : PFT_BLOCK, 0) != hipSuccess || b < 1) b = 1;
  n = b;
  return n;
}

static int stage_occupancy(int stage, int mode, int gls, int kind)
{
  return with_stage(stage, [&](auto st) {
    return with_mode(mode, [&](auto m) {
      return with_bool(gls, [&](auto g) {
        return kernel_occupancy<decltype(st)::value, decltype(m)::value, decltype(g)::value>(kind);
      });
    });
  });
}

static void launch_stage(int stage, int mode, int gls, int kind, dim3 g, hipStream_t st, const StageArgs& a,
                         const pft_consts& c)
{
  with_stage(stage, [&](auto sv) {
    with_mode(mode, [&](auto mv) {
      with_bool(gls, [&](auto gv) {
        constexpr int STAGE = decltype(sv)::value, MODE = decltype(mv)::value;
        constexpr bool GLS = decltype(gv)::value;
        if (kind == KFUSED) {
          merson_fused<STAGE, MODE, GLS><<<g, PFT_FBLOCK, 0, st>>>(a, c);
        } else {
          merson_stage<STAGE, MODE, GLS><<<g, PFT_BLOCK, 0, st>>>(a, c);
        }
      });
    });
  });
}

// a launch's plan (slab_plan) into its kernel arguments (StageArgs, PairArgs) and into the record of
// pft_slab_launch_geometry (rec 1..5: the stage the launch ends)
template <class A>
static void plan_apply(pft_slab* s, int rec, const pft_zplan& p, A& a)
{
  a.k_begin = p.k_begin;
  a.k_end = p.k_end;
  a.kz = p.kz;
  a.kspan = p.kspan;
  a.nchunk = p.nchunk;
  a.nbw = p.nbw;
  a.bends = p.bends;
  a.c0 = p.c0;
  a.nint = p.nint;
  if (p.inl) a.bdone = s->bdone;
  if (rec < 1) return;
  s->launch_nwg[rec] = p.nbw + p.nint;
  s->launch_kz[rec] = p.kz;
  s->launch_ntile[rec] = a.ntile;
  s->launch_bnd[rec] = p.bnd;
}

// a planned launch on its stream, with what follows it.  beside: a boundary launch on the boundary
// stream, behind what the compute stream holds, so that it runs beside the interior launch.
template <class F>
static int launch_planned(pft_slab* s, const pft_zplan& p, bool beside, F&& launch)
{
  hipStream_t st = s->stream;
  if (beside) {
    HIPCHK(hipEventRecord(s->ev_pre, s->stream));
    HIPCHK(hipStreamWaitEvent(s->bnd, s->ev_pre, 0));
    st = s->bnd;
  }
  launch(st);
  HIPCHK(hipGetLastError());
  if (beside) {
    HIPCHK(hipEventRecord(s->ev_bnd, s->bnd));
    s->bnd_pending = 1;
  }
  if (p.inl) {
    s->bdone_target += (unsigned long long)p.nbw;
    s->inline_pending = 1;
    // the copies' trigger, on the comm stream at once: queued now, it is normally dispatched while
    // the previous launch still runs and sits on its CU before this launch fills the chip (pair 4+5
    // at 256 VGPRs leaves no room beside its workgroups: a trigger queued later waited for a CU
    // until this launch drained -- the copies then ran after it)
    if (s->trig_early) {
      slab_trigger(s);
      HIPCHK(hipGetLastError());
    }
  }
  return 0;
}

extern "C" {

// merson_fused tile: wx cell pairs x ty rows, 256 threads.  Limits: wx * ty <= 256 threads, the
// halo ring (2 wx + 4 + 2 ty pairs per field, 3 fields) loaded by one pass of the 256 threads,
// (2 wx + 4)(ty + 2) <= PFT_FUSED_LF doubles of LDS per field and plane.
static bool fused_geometry_ok(int wx, int ty)
{
  return wx >= 4 && ty >= 1 && wx * ty <= PFT_FBLOCK && 3 * (2 * wx + 4 + 2 * ty) <= PFT_FBLOCK &&
         (2 * wx + 4) * (ty + 2) <= PFT_FUSED_LF;
}

// automatic choice: 16..40 pairs wide (rows of 256-640 B), the tallest rows count that fits, and
// of those the tile whose workgroups carry the fewest idle lanes over the whole plane (edge tiles,
// threads beyond wx * ty); within 0.5% the wider.  Measured: with 64 x 8 tiles at n1 = 200 a
// quarter of the workgroups are 7/8 idle; a z-march of 64-wide tiles streams at 4.7-4.9 TB/s
// there and at 5.2-5.4 TB/s when n1 is a multiple of 64 (scripts/probes/stream_probe.hip).
// n1 = 200 and 400: 25 x 10 pairs (50 x 10 cells), all lanes but 6 busy.
static double fused_geometry(int n1, int n2, int* wx_out, int* ty_out)
{
  const int np = n1 / 2;
  double best = -1.0;
  int bw = 32, bt = 8;
  for (int wx = 16; wx <= 40; ++wx) {
    int ty = PFT_FBLOCK / wx;
    while (ty > 1 && !fused_geometry_ok(wx, ty)) --ty;
    if (!fused_geometry_ok(wx, ty)) continue;
    const long lanes = (long)((np + wx - 1) / wx) * ((n2 + ty - 1) / ty) * PFT_FBLOCK;
    const double eff = (double)np * n2 / (double)lanes;
    if (eff >= best - 0.005) {
      if (eff > best) best = eff;
      bw = wx;
      bt = ty;
    }
  }
  *wx_out = bw;
  *ty_out = bt;
  return best;   // busy lanes / launched lanes over the plane
}

// fused_geometry of the slab's plane, computed once (slab_kind and every launch ask for it)
static double slab_fgeo(const pft_slab* cs, int* wx, int* ty)
{
  pft_slab* s = const_cast<pft_slab*>(cs);
  if (!s->fgeo_valid) {
    s->fgeo_eff = fused_geometry(s->d.n1, s->d.n2, &s->fgeo_wx, &s->fgeo_ty);
    s->fgeo_valid = 1;
  }
  *wx = s->fgeo_wx;
  *ty = s->fgeo_ty;
  return s->fgeo_eff;
}

// z-chunk count memo: the cost model (pft_zplan_kz) scans every chunk count (400 planes: 400
// candidates); its result only depends on its arguments, all of them in the key.  One slot per
// launcher and chunking rule (plain, or ends-first's min_nch = 3): pft_slab::kz_memo.
enum { KZ_STAGE = 0 /* + stage + 6 gls */, KZ_PAIR = 12 /* + (first == 4) */ };
static int chunk_kz(void* memo, int occ, long ntile, int nplanes, int min_nch, int ncu)
{
  pft_slab::KzMemo* m = (pft_slab::KzMemo*)memo + (min_nch >= 3 ? 1 : 0);
  const long key = (((long)min_nch << 56) ^ ((long)occ << 52) ^ ((long)ncu << 40) ^ (ntile << 24) ^ (long)nplanes) + 1;
  if (m->key != key) {
    m->kz = pft_zplan_kz(occ, ntile, nplanes, min_nch, ncu);
    m->key = key;
  }
  return m->kz;
}

// the plan of a launch (pft_zplan.h) on this slab: its forced kz, the compute stream's CUs (launches
// on it chunk here) and the memo
static int slab_plan(pft_slab* s, pft_zplan* p, int launcher, int k_begin, int k_end, int ntile, int occ,
                     int depths, bool can_inline)
{
  const pft_zplan_in in = {k_begin, k_end, s->d.n3, ntile, s->kz, occ, s->n_cu - s->cu_reserved,
                           depths, can_inline ? 1 : 0, chunk_kz, s->kz_memo[launcher]};
  return pft_zplan_make(p, &in);
}

static int slab_kind(const pft_slab* s)
{
  // 16-byte rows need n1 even; the aux-array path (recompute off) is the cache kernel's.  (An
  // LDS-tiled aux-array kernel, 72 doubles per cell-step, was removed: measured slower than the
  // recompute kernel everywhere)
  if (s->d.n1 % 2 != 0 || s->tile_wx == 0 || !s->recompute) return KCACHE;
  // automatic choice: the LDS-tiled kernel unless its tiles leave most lanes idle (planes
  // narrower than a tile, e.g. n1 < 32); the cache kernel's flat 256-cell workgroups fit any
  // plane.  Measured at 100^3 (50 x 50 x 100, 25 x 10-pair tiles fit exactly): 4 810 vs 3 980
  // Mcells*steps/s (47 vs 60 us per attempted step untimed)
  if (s->tile_wx == 1) {
    int wx, ty;
    if (slab_fgeo(s, &wx, &ty) < 0.7) return KCACHE;
  }
  return KFUSED;
}

int pft_slab_stage_output(const pft_slab* s, int stage)
{
  // the buffer each stage of the step writes (and whose boundary planes neighbours need)
  static const int aux_out[6] = {-1, PFT_BUF_A0, PFT_BUF_A1, PFT_BUF_A0, PFT_BUF_A1, PFT_BUF_XN};
  static const int rc_out[6] = {-1, PFT_BUF_K1, PFT_BUF_A0 /* K2 */, PFT_BUF_K3, PFT_BUF_K4, PFT_BUF_XN};
  if (stage < 1 || stage > 5) return -2;
  return slab_kind(s) == KFUSED ? rc_out[stage] : aux_out[stage];
}

int pft_slab_tile_geometry(const pft_slab* s, int stage, int* wx, int* ty)
{
  const int kind = slab_kind(s);
  const bool auto_tile = s->tile_wx == 1 || s->tile_wx == 2;
  if (kind == KCACHE) {
    *wx = 0;
    *ty = 0;
  } else if (auto_tile) {
    slab_fgeo(s, wx, ty);
  } else {
    *wx = s->tile_wx;
    *ty = PFT_FBLOCK / *wx;
  }
  return kind;
}

int pft_slab_launch_geometry(const pft_slab* s, int stage, int* nwg, int* kz, int* ntile)
{
  if (stage < 1 || stage > 5 || !s->launch_nwg[stage]) return -2;
  *nwg = s->launch_nwg[stage];
  *kz = s->launch_kz[stage];
  *ntile = s->launch_ntile[stage];
  return s->launch_bnd[stage] ? 1 : 0;
}

int pft_xcd_remap(int b, int n) { return xcd_remap(b, n); }

int pft_slab_eps_route(const pft_slab* s)
{
  if (!s->launch_nwg[5]) return -2;
  return s->launch_part ? 1 : 0;
}

int pft_slab_stage_fields(const pft_slab* s, int stage)
{
  // fields of a stage's output buffer that the stage writes (stage 6: the speculative stage 1):
  // gl is not evolved under gl_static, and its K's are literal zeros on the recompute path
  if (stage < 1 || stage > 6) return -2;
  if (s->d.gl_static) return 2;
  if (slab_kind(s) == KFUSED && stage != 5) return 2;
  // stage 5 with gl_keep (agreed by every rank, rk_solver.c): gl's x(t+h) is not stored; the
  // neighbours' XN gl ghost planes already equal X's (both exchanged at upload)
  if (stage == 5 && pft_slab_get_gl_keep(s) && slab_kind(s) == KFUSED) return 2;
  return 3;
}

// arm the publication of an error-norm launch of nwg workgroups: the next slot of the host's ring
// pre-set to the sentinel (here, before the launch; the host polls it in pft_slab_eps_fetch), and
// the deferred publication into it -- the launch's workgroups store partials (eps_store_part), the
// next stage-1 launch reduces and publishes them.  cap_nwg: partials to make room for now.
static int pub_arm(pft_slab* s, long nwg, unsigned long long** part, long cap_nwg = 0)
{
  const int j = (int)(s->pub_next % PFT_PUB_SLOTS);
  __atomic_store_n(&s->pub_ring[2 * j], PFT_PUB_SENTINEL, __ATOMIC_RELEASE);
  __atomic_store_n(&s->pub_ring[2 * j + 1], PFT_PUB_SENTINEL, __ATOMIC_RELEASE);
  if (std::max(nwg, cap_nwg) > s->part_cap) {
    if (s->part) HIPCHK(hipFree(s->part));
    s->part = nullptr;
    s->part_cap = 0;
    const long cap = std::max(std::max(nwg, cap_nwg), 4096L);
    HIPCHK(hipMalloc((void**)&s->part, 16 * (size_t)cap));
    s->part_cap = cap;
  }
  s->defer_n = (int)nwg;
  s->defer_slot = j;
  *part = s->part;
  return 0;
}

static int run_stage(pft_slab* s, int stage, const double* in, double* kout, double* out, double t_stage,
                     double coef, double h, int k_begin, int k_end, int gls, int kind)
{
  const int mode = s->d.calc_mode;
  if (mode != 0 && mode != 1 && mode != 2 && mode != 10 && mode != 11) return -2;
  StageArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in;
  a.x = s->buf[PFT_BUF_X];
  a.k1 = s->buf[PFT_BUF_K1];
  a.k2 = s->buf[PFT_BUF_A0];
  a.k3 = s->buf[PFT_BUF_K3];
  a.k4 = s->buf[PFT_BUF_K4];
  a.kout = kout;
  a.out = out;
  a.noise = s->noise;
  a.eps_bits = s->scratch;
  a.nonfinite = (unsigned int*)(s->scratch + 1);
  a.fs = s->fs;
  a.n1 = s->d.n1;
  a.n2 = s->d.n2;
  a.n3 = s->d.n3;
  a.plane = s->plane;
  a.has_below = s->d.has_below;
  a.has_above = s->d.has_above;
  // tile: tile_wx 1 / 2 = automatic (fused_geometry), else that many pairs per row
  const bool auto_tile = s->tile_wx == 1 || s->tile_wx == 2;
  if (kind == KFUSED) {
    if (auto_tile) {
      slab_fgeo(s, &a.gwx, &a.gty);
    } else {
      a.gwx = s->tile_wx;
      a.gty = PFT_FBLOCK / s->tile_wx;
    }
    if (!fused_geometry_ok(a.gwx, a.gty)) return -2;
    a.ntile = ((s->d.n1 + 2 * a.gwx - 1) / (2 * a.gwx)) * ((s->d.n2 + a.gty - 1) / a.gty);
  } else {
    a.ntile = (s->plane + PFT_BLOCK - 1) / PFT_BLOCK;
  }
  // the z-chunks.  Measured at 400^3 (80 tiles): stage 5 (occ 2) 6 chunks, 0.348 ms vs 0.393 for 16;
  // stage 1 16 chunks of 25 planes, 0.153 ms vs 0.163 for 9 of 45 (the cost model's own choice for
  // occ 3 is 9 of 45).  On a 400 x 400 x 100 slab (320 tiles, one 800^3 8-way rank) stages 4-5: 3
  // chunks (960 workgroups, 2 rounds) 0.261 / 0.349 ms against 0.314 / 0.436 for one round of 320
  // (64 CUs with 2 workgroups, 192 with 1).
  // Boundary launches of either depth; the inline boundary is merson_fused's, never gated.
  pft_zplan p;
  const int prc = slab_plan(s, &p, KZ_STAGE + stage + 6 * (gls ? 1 : 0), k_begin, k_end, a.ntile,
                            stage_occupancy(stage, mode, gls, kind), 1 | 2,
                            kind == KFUSED && s->bdone && !s->gate_use_seq);
  if (prc <= 0) return prc;
  const bool bnd = p.bnd != 0;
  plan_apply(s, stage, p, a);
  a.shards = s->eps_shards + (bnd ? PFT_EPS_SHARDS : 0);
  a.T_top = t_stage < s->c.phase_switch_time ? s->c.top_temp1 : s->c.top_temp2;
  a.coef = coef;
  a.h = h;
  a.cin = pft_stepctl_stage(stage, 0.0, h).cin;   // the recompute path rebuilds the stage input
  if (kind == KFUSED && in) a.x = in;    // pure RHS / speculative stage 1: the input is the given buffer
  // gl's x(t+h) is x + coef*(0.5*(0.0 + 0.0) + 2.0*0.0) (gl's K's are literal zeros): equal to x
  // bit for bit when coef is finite and no gl value is -0.0 or NaN, which the solver checked at
  // upload (pft_slab_set_gl_keep); XN's gl then already holds it, and stage 5 skips that store
  a.gl_keep = stage == 5 && kind == KFUSED && out && s->gl_keep && std::isfinite(coef) ? 1 : 0;
  if (kind == KFUSED && s->gate_use_seq) {
    // gated (pft_slab_gate_use): the scalars above are the launch's own (gate_scalars), from the
    // decision the host has not taken yet; the kernel ANDs isfinite(coef) into gl_keep
    const int j = (int)(s->gate_use_seq % PFT_GATE_SLOTS);
    a.gate = s->gate_dev + 4 * j;
    a.gseq = s->gate_use_seq;
    a.gl_keep = stage == 5 && out && s->gl_keep ? 1 : 0;
  }
  a.em0 = s->d.eps_mult[0];
  a.em1 = s->d.eps_mult[1];
  a.em2 = s->d.eps_mult[2];
  s->pub_armed = 0;
  if (stage == 5 && kind == KFUSED && out && !bnd && p.k_begin == 0 && p.k_end == s->d.n3 && s->inkernel_pub) {
    // the whole slab in one launch: its error norm is published for the host
    if (int rc = pub_arm(s, (long)a.ntile * a.nchunk, &a.part)) return rc;
    s->pub_armed = 1;
    s->pub_slot = s->defer_slot;
  }
  dim3 g((unsigned)(a.nbw + a.nint));
  if (stage == 5) s->launch_part = a.part != nullptr;
  bool extra = false;
  // a stage launch's interior fills the chip: its boundary runs beside it only in bnd_mode 1 (slower:
  // the two launches' workgroups are dealt interleaved and the interior ends late).  In the boundary
  // pipeline (bnd_mode 3) the halo waits are on the boundary stream: a stage launch's boundary on
  // the compute stream first joins it
  const bool beside = bnd && s->bnd_mode == 1;
  if (bnd && s->bnd_mode == 3 && s->bnd) {
    HIPCHK(hipEventRecord(s->ev_join, s->bnd));
    HIPCHK(hipStreamWaitEvent(s->stream, s->ev_join, 0));
  }
  if (stage == 1 && kind == KFUSED && s->defer_n > 0) {
    // the previous error-norm launch's partials: reduced and published by one extra workgroup
    a.part = s->part;
    a.npart = s->defer_n;
    a.pub = s->pub_ring_dev + 2 * s->defer_slot;
    s->defer_n = 0;
    extra = true;
  }
  if (stage == 1 && kind == KFUSED && s->gate_arm_seq && in) {
    // the speculative stage 1 armed by pft_slab_gate_arm: its extra workgroup also decides the
    // step that just ended, for the next step's pre-enqueued launches and for the host
    const int j = (int)(s->gate_arm_seq % PFT_GATE_SLOTS);
    a.gpin = s->gate_pin_dev + 4 * j;
    a.gdev = s->gate_dev + 4 * j;
    a.gdec_seq = s->gate_arm_seq;
    a.dt = s->gate_arm_t;
    a.dh = s->gate_arm_h;
    a.k = s->gate_k;
    a.d_flip = s->gate_flip;
    __atomic_store_n(&s->gate_pin[4 * j], 0ULL, __ATOMIC_RELEASE);   // no decision yet
    s->gate_arm_seq = 0;
    extra = true;
  }
  if (extra) g.x += 1;
  if (int rc = launch_planned(s, p, beside, [&](hipStream_t st) { launch_stage(stage, mode, gls, kind, g, st, a, s->c); }))
    return rc;
  if (bnd && !beside) s->bnd_split = 1;   // a boundary launch before its interior on the compute stream
  return 0;
}

int pft_slab_stage(pft_slab* s, int stage, double t_stage, double coef, double h, int k_begin, int k_end)
{
  if (stage < 1 || stage > 5) return -2;
  const int kind = slab_kind(s);
  if (kind == KFUSED) {
    // inputs rebuilt from x, K1, K2 (in A0), K3, K4; outputs K_stage or x(t+h)
    static const int k_of[6] = {-1, PFT_BUF_K1, PFT_BUF_A0, PFT_BUF_K3, PFT_BUF_K4, -1};
    return run_stage(s, stage, nullptr, k_of[stage] >= 0 ? s->buf[k_of[stage]] : nullptr,
                     stage == 5 ? s->buf[PFT_BUF_XN] : nullptr, t_stage, coef, h, k_begin, k_end,
                     s->d.gl_static, kind);
  }
  // aux path: in -> (kout, out)
  static const int in_of[6] = {-1, PFT_BUF_X, PFT_BUF_A0, PFT_BUF_A1, PFT_BUF_A0, PFT_BUF_A1};
  static const int out_of[6] = {-1, PFT_BUF_A0, PFT_BUF_A1, PFT_BUF_A0, PFT_BUF_A1, PFT_BUF_XN};
  static const int k_of[6] = {-1, PFT_BUF_K1, -1, PFT_BUF_K3, PFT_BUF_K4, -1};
  return run_stage(s, stage, s->buf[in_of[stage]], k_of[stage] >= 0 ? s->buf[k_of[stage]] : nullptr,
                   s->buf[out_of[stage]], t_stage, coef, h, k_begin, k_end, s->d.gl_static, kind);
}

int pft_slab_rhs(pft_slab* s, int in_buf, int out_buf, double t)
{
  if (in_buf < 0 || in_buf >= PFT_BUF_COUNT || out_buf < 0 || out_buf >= PFT_BUF_COUNT) return -2;
  return run_stage(s, 0, s->buf[in_buf], s->buf[out_buf], nullptr, t, 0.0, 0.0, -1, -1, 0, slab_kind(s));
}

int pft_slab_set_gl_keep(pft_slab* s, int on)
{
  s->gl_keep = on ? 1 : 0;
  return 0;
}

int pft_slab_get_gl_keep(const pft_slab* s) { return s->gl_keep; }

int pft_slab_set_recompute(pft_slab* s, int on)
{
  s->recompute = on ? 1 : 0;
  return 0;
}

int pft_slab_set_consts(pft_slab* s, const pft_consts* c)
{
  s->c = *c;
  return slab_div_consts(s);
}

int pft_div_alpha_check(double alpha, unsigned long long n_hashed, const unsigned long long* list,
                        unsigned long long n_list, unsigned long long* mismatches)
{
  pft_consts c;
  memset(&c, 0, sizeof(c));
  c.alpha = alpha;
  double* dc = nullptr;
  unsigned long long *dl = nullptr, *db = nullptr;
  *mismatches = ~0ULL;
  if (n_hashed + n_list > (1ULL << 31) || (n_list && !list)) return -2;
  hipError_t e = hipMalloc((void**)&dc, sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&db, 8);
  if (e == hipSuccess && n_list) e = hipMalloc((void**)&dl, 8 * (size_t)n_list);
  if (e == hipSuccess && n_list) e = hipMemcpy(dl, list, 8 * (size_t)n_list, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(db, 0, 8);
  if (e == hipSuccess) {
    div_alpha_consts_kernel<<<1, 1>>>(alpha, dc);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(&c.ralpha, dc, sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    const unsigned long long n = n_hashed + n_list;
    if (n) {
      div_alpha_check_kernel<<<(unsigned)((n + 255) / 256), 256>>>(c, n_hashed, dl, n_list, db);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipMemcpy(mismatches, db, 8, hipMemcpyDeviceToHost);
  if (dc) (void)hipFree(dc);
  if (dl) (void)hipFree(dl);
  if (db) (void)hipFree(db);
  if (e != hipSuccess) return fail(e, "pft_div_alpha_check");
  return 0;
}

int pft_cosh_eval(const double* x, double* y, unsigned long long n)
{
  if (n > (1ULL << 31) || (n && (!x || !y))) return -2;
  if (!n) return 0;
  double *dx = nullptr, *dy = nullptr;
  const size_t bytes = sizeof(double) * (size_t)n;
  hipError_t e = hipMalloc((void**)&dx, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&dy, bytes);
  if (e == hipSuccess) e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    cosh_eval_kernel<<<(unsigned)((n + 255) / 256), 256>>>(dx, dy, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(y, dy, bytes, hipMemcpyDeviceToHost);
  if (dx) (void)hipFree(dx);
  if (dy) (void)hipFree(dy);
  if (e != hipSuccess) return fail(e, "pft_cosh_eval");
  return 0;
}

int pft_slab_set_eps_mult(pft_slab* s, const double* em3)
{
  for (int q = 0; q < 3; ++q) s->d.eps_mult[q] = em3[q];
  return 0;
}

int pft_slab_set_noise(pft_slab* s, const double* host_noise)
{
  if (!host_noise) {
    if (s->noise) HIPCHK(hipFree(s->noise));
    s->noise = nullptr;
    return 0;
  }
  const size_t bytes = sizeof(double) * (size_t)s->plane * s->d.n3;
  if (!s->noise) HIPCHK(hipMalloc((void**)&s->noise, bytes));
  HIPCHK(hipMemcpy(s->noise, host_noise, bytes, hipMemcpyHostToDevice));
  return 0;
}

int pft_slab_order(pft_slab* s, int comm_first)
{
  // the second stream waits for the work enqueued so far on the first
  hipStream_t from = comm_first ? s->comm : s->stream, to = comm_first ? s->stream : s->comm;
  hipEvent_t ev = s->ev_order[comm_first ? 1 : 0];
  HIPCHK(hipEventRecord(ev, from));
  HIPCHK(hipStreamWaitEvent(to, ev, 0));
  return 0;
}

int pft_slab_eps_reset(pft_slab* s)
{
  HIPCHK(hipMemsetAsync(s->scratch, 0, 16, s->stream));
  return 0;
}

int pft_slab_eps_mark(pft_slab* s) { return pft_slab_eps_mark_on(s, (void*)s->stream); }

int pft_slab_set_inkernel_publish(pft_slab* s, int on)
{
  s->inkernel_pub = on ? 1 : 0;
  s->pub_armed = 0;
  s->split_pub = 0;
  s->defer_n = 0;
  return 0;
}

int pft_slab_eps_mark_on(pft_slab* s, void* stream)
{
  if (s->split_pub) {
    // a split stage 4+5 whose interior launch had no planes: the boundary's partials are all
    s->split_pub = 0;
    s->pub_armed = 1;
    s->pub_slot = s->defer_slot;
  }
  if (s->pub_armed && stream == (void*)s->stream) {
    // the stage-5 launch just enqueued publishes the error norm itself
    s->pub_armed = 0;
    s->pub_next++;
    s->eps_marked = 2;
    return 0;
  }
  // the error norm goes to coherent pinned host memory by a one-thread kernel (which also resets
  // it for the next step), and an event marks its completion: the host waits for that event
  // only, never for a copy queued behind (or beside) the speculative stage-1 kernel that follows
  // on the compute stream
  publish_kernel<<<1, 1, 0, (hipStream_t)stream>>>(s->scratch, s->host_pub_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(s->ev_eps, (hipStream_t)stream));
  s->eps_marked = 1;
  return 0;
}

int pft_slab_eps_fetch(pft_slab* s, double* eps, int* nonfinite)
{
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_eps_fetch");
  if (s->eps_marked == 2) {
    // published beside the speculative stage 1 (deferred publication): poll the slot (pinned,
    // coherent) until both words left the sentinel while that kernel keeps running.  Without a
    // stage-1 launch since the error-norm launch, a one-workgroup reduction publishes instead.
    s->eps_marked = 0;
    if (s->defer_n > 0) {
      eps_reduce_kernel<<<1, 256, 0, s->stream>>>(s->part, s->defer_n, s->pub_ring_dev + 2 * s->defer_slot);
      s->defer_n = 0;
      HIPCHK(hipGetLastError());
    }
    volatile unsigned long long* w = s->pub_ring + 2 * s->pub_slot;
    long spins = 0;
    double t0 = 0.0;
    while (__atomic_load_n(&w[0], __ATOMIC_ACQUIRE) == PFT_PUB_SENTINEL ||
           __atomic_load_n(&w[1], __ATOMIC_ACQUIRE) == PFT_PUB_SENTINEL) {
      if (++spins < 200000) {
        __builtin_ia32_pause();
      } else if ((spins & 1023) == 0) {
        // long wait: make sure the stream is alive (a fault ends here with its error), and that an
        // ipc neighbour's halo has not been missing for longer than the slab's timeout
        const hipError_t q = hipStreamQuery(s->stream);
        if (q != hipSuccess && q != hipErrorNotReady) return fail(q, "hipStreamQuery (error norm poll)");
        if (q == hipSuccess && __atomic_load_n(&w[1], __ATOMIC_ACQUIRE) == PFT_PUB_SENTINEL)
          return fail(hipErrorUnknown, "error norm never published");
        if (s->watch) {
          const int rc = slab_watch(s, &t0, "error norm poll");
          if (rc) return rc;
        } else if (s->peer[0].on || s->peer[1].on) {
          if (t0 == 0.0) t0 = wall_s();
          else if (wall_s() - t0 > s->timeout_s) return slab_timed_out(s, "error norm poll");
        }
        sched_yield();
      }
    }
    s->host_scratch[0] = w[0];
    s->host_scratch[1] = w[1];
  } else if (s->eps_marked) {
    // read back on the side stream: work enqueued on the compute stream after the mark (the
    // speculative stage 1 of the next step) keeps running while the host decides
    s->eps_marked = 0;
    int rc = slab_wait(s, s->ev_eps, "error norm event");
    if (rc) return rc;
    s->host_scratch[0] = __atomic_load_n(&s->host_pub[0], __ATOMIC_ACQUIRE);
    s->host_scratch[1] = __atomic_load_n(&s->host_pub[1], __ATOMIC_ACQUIRE);
  } else {
    HIPCHK(hipMemcpyAsync(s->host_scratch, s->scratch, 16, hipMemcpyDeviceToHost, s->stream));
    int rc = slab_wait(s, nullptr, "error norm read-back");
    if (rc) return rc;
  }
  unsigned long long b = s->host_scratch[0];
  double v;
  memcpy(&v, &b, 8);
  *eps = v;
  if (nonfinite) *nonfinite = (int)(s->host_scratch[1] & 0xffffffffu);
  return 0;
}

static int timing_collect(pft_slab* s, bool wait)
{
  for (int st = 1; st <= 5; ++st) {
    while (s->ttail[st] < s->thead[st]) {
      hipEvent_t* ev = s->tev[st][s->ttail[st] % PFT_TRING];
      if (wait) {
        HIPCHK(hipEventSynchronize(ev[1]));
      } else {
        const hipError_t q = hipEventQuery(ev[1]);
        if (q == hipErrorNotReady) break;
        if (q != hipSuccess) return fail(q, "hipEventQuery");
      }
      float e = 0.f;
      HIPCHK(hipEventElapsedTime(&e, ev[0], ev[1]));
      s->tacc_ms[st] += (double)e;
      s->tacc_n[st] += 1;
      s->ttail[st]++;
    }
  }
  return 0;
}

static void timing_hand_out(pft_slab* s, double* ms, long* n)
{
  for (int st = 1; st <= 5; ++st) {
    ms[st] += s->tacc_ms[st];
    n[st] += s->tacc_n[st];
    s->tacc_ms[st] = 0.0;
    s->tacc_n[st] = 0;
  }
}

int pft_slab_timing_mark(pft_slab* s, int stage, int end)
{
  if (stage < 1 || stage > 5) return -2;
  if (!end && s->thead[stage] - s->ttail[stage] >= PFT_TRING) {
    int rc = timing_collect(s, true);   // ring full: read the oldest pairs before re-recording them
    if (rc) return rc;
  }
  hipEvent_t* ev = s->tev[stage][s->thead[stage] % PFT_TRING];
  if (!ev[0]) {
    HIPCHK(hipEventCreate(&ev[0]));
    HIPCHK(hipEventCreate(&ev[1]));
  }
  HIPCHK(hipEventRecord(ev[end ? 1 : 0], s->stream));
  if (end) s->thead[stage]++;
  return 0;
}

int pft_slab_timing_collect(pft_slab* s, double* ms, long* n)
{
  int rc = timing_collect(s, false);
  timing_hand_out(s, ms, n);
  return rc;
}

int pft_slab_timing_flush(pft_slab* s, double* ms, long* n)
{
  int rc = timing_collect(s, true);
  timing_hand_out(s, ms, n);
  return rc;
}

int pft_slab_can_speculate(const pft_slab* s) { return slab_kind(s) == KFUSED; }

// ---- gated steps (f4) ------------------------------------------------------------------------
// the device's x^0.2 correction (pow02_fix) compiled for the host: CPU tests check it against a
// high-precision reference with candidates one ulp off either way (tests/test_pow02.py)
double pft_pow02_fix(double x, double c) { return pow02_fix(x, c); }

int pft_slab_gate_config(pft_slab* s, double final_time, double delta, double h_min, int delta_local, int handle_nan)
{
  s->gate_k = pft_stepctl_consts{final_time, delta, h_min, delta_local, handle_nan};
  return 0;
}

unsigned long long pft_slab_gate_arm(pft_slab* s, double t, double h)
{
  s->gate_arm_seq = ++s->gate_seq;
  s->gate_arm_t = t;
  s->gate_arm_h = h;
  return s->gate_arm_seq;
}

int pft_slab_gate_decision(pft_slab* s, unsigned long long seq, int* go, double* t, double* h)
{
  // the device's decision (gate_decide), published right after the error norm the host has read
  volatile unsigned long long* w = s->gate_pin + 4 * (seq % PFT_GATE_SLOTS);
  long spins = 0;
  unsigned long long v;
  while (((v = __atomic_load_n(&w[0], __ATOMIC_ACQUIRE)) & ~PFT_GATE_SKIP) != seq) {
    if (++spins < 200000) {
      __builtin_ia32_pause();
    } else if ((spins & 1023) == 0) {
      const hipError_t q = hipStreamQuery(s->stream);
      if (q != hipSuccess && q != hipErrorNotReady) return fail(q, "hipStreamQuery (gate decision poll)");
      if (q == hipSuccess && ((__atomic_load_n(&w[0], __ATOMIC_ACQUIRE) & ~PFT_GATE_SKIP) != seq))
        return fail(hipErrorUnknown, "gate decision never published");
      sched_yield();
    }
  }
  *go = v == seq;
  const unsigned long long tb = w[1], hb = w[2];
  memcpy(t, &tb, 8);
  memcpy(h, &hb, 8);
  return 0;
}

int pft_slab_gate_use(pft_slab* s, unsigned long long seq)
{
  s->gate_use_seq = seq;
  return 0;
}

int pft_slab_book_save(pft_slab* s, int which)
{
  if (which < 0 || which > 1) return -2;
  pft_slab::Book& b = s->book[which];
  b.pub_next = s->pub_next;
  b.pub_armed = s->pub_armed;
  b.pub_slot = s->pub_slot;
  b.eps_marked = s->eps_marked;
  b.defer_n = s->defer_n;
  b.defer_slot = s->defer_slot;
  return 0;
}

int pft_slab_book_load(pft_slab* s, int which)
{
  if (which < 0 || which > 1) return -2;
  const pft_slab::Book& b = s->book[which];
  // pub_next only moves forward: a discarded gated launch may still publish into its slot
  s->pub_next = std::max(s->pub_next, b.pub_next);
  s->pub_armed = b.pub_armed;
  s->pub_slot = b.pub_slot;
  s->eps_marked = b.eps_marked;
  s->defer_n = b.defer_n;
  s->defer_slot = b.defer_slot;
  return 0;
}

int pft_slab_stage_spec(pft_slab* s, double t_stage, int k_begin, int k_end)
{
  // stage 1 of the next step, K1' = f(t + h, x(t + h)), from XN into A1 (unused on the recompute
  // path) -- before the accept decision is known
  if (slab_kind(s) != KFUSED) return -2;
  return run_stage(s, 1, s->buf[PFT_BUF_XN], s->buf[PFT_BUF_A1], nullptr, t_stage, 0.0, 0.0, k_begin, k_end,
                   s->d.gl_static, KFUSED);
}

}  // extern "C"

// ---- pair kernels (merson_pair): stages 2+3 and 4+5 of a step, one launch each -------------

static void launch_pair(int first, int mode, bool glx, int lwp, dim3 g, hipStream_t st, const PairArgs& a,
                        const pft_consts& c)
{
  with_bool(first == 2, [&](auto fv) {
    with_mode(mode, [&](auto mv) {
      with_bool(glx, [&](auto gv) {
        with_bool(lwp == 12, [&](auto lv) {
          constexpr int SA = decltype(fv)::value ? 2 : 4, MODE = decltype(mv)::value;
          constexpr int LWP = decltype(lv)::value ? 12 : 22;
          constexpr bool GLX = decltype(gv)::value;
          merson_pair<SA, MODE, GLX, LWP><<<g, PFT_PBLOCK, 0, st>>>(a, c);
        });
      });
    });
  });
}

// resident workgroups per CU of a pair kernel (hipOccupancy..., cached; the 22-pair pitch's, gl
// from its own input)
template <int SA, int MODE>
static int pair_kernel_occupancy()
{
  static int n = 0;
  if (n) return n;
  int b = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, (const void*)merson_pair<SA, MODE, false, 22>, PFT_PBLOCK, 0) != hipSuccess || b < 1) b = 1;
  n = b;
  return n;
}

static int pair_occupancy(int first, int mode)
{
  return with_bool(first == 2, [&](auto fv) {
    return with_mode(mode, [&](auto mv) {
      return pair_kernel_occupancy<decltype(fv)::value ? 2 : 4, decltype(mv)::value>();
    });
  });
}

// the LDS row pitch (pairs) of a pair tile tx cells wide: 12 up to 20 cells, 22 up to 40
static int pair_lwp(int tx) { return tx <= 20 ? 12 : 22; }

// pair tile: tx cells (even) x ty rows; its R2 positions ((tx/2 + 2) pairs x (ty + 4) rows) one
// per thread, and the two LDS plane rings (rows of pair_lwp(tx) slots) within their halves
static bool pair_geometry_ok(int tx, int ty)
{
  const int lwp = pair_lwp(tx);
  // positions: one per thread, and up to PFT_PAIR_NEX more in the last ring row (loaded by
  // the last lanes of the last wave beside their own: merson_pair)
  return tx >= 2 && tx % 2 == 0 && ty >= 1 &&
         (tx / 2 + 2) * (ty + 4) <= (lwp == 22 ? PFT_PBLOCK + PFT_PAIR_NEX : PFT_PBLOCK) &&
         (tx / 2 + 2) * (ty + 3) <= PFT_PBLOCK && tx / 2 + 2 <= 22 &&
         2 * PFT_PAIR_PADP + lwp * (ty + 4) <= PFT_PAIR_H && 2 * PFT_PAIR_PADP + lwp * (ty + 2) <= PFT_PAIR_HB &&
         (tx / 2) * ty <= PFT_PAIR_OPN;
}

// automatic tile: the fewest workgroups per plane (a workgroup-plane costs about the same whatever
// the tile's edge tiles hold), of those the one with the fewest idle tile cells, then the wider.
// n1 = 200 / 400: 40 x 20 cells (5 x 10 / 10 x 20 tiles, 484 of 512 threads evaluate stage A and
// 400 stage B, 16 positions of the last ring row loaded by load-only lanes; 40 x 19 before round 6); n1 = 100: 20 x 34 cells (5 x 3 tiles, 98% of their cells in the plane, against 18
// 34 x 19 tiles with the 22-pair pitch alone).  Returns the tiles per plane, 0 when no tile fits
// (n1 odd).
static long pair_geometry(int n1, int n2, int* tx_out, int* ty_out)
{
  long best = 0, best_idle = 0;
  int bx = 0, by = 0, bleg = 0;
  if (n1 < 2 || n1 % 2 || n2 < 1) return 0;
  for (int tx = 2; tx <= n1 + 1 && tx <= 40; tx += 2) {
    for (int ty = std::min(n2, PFT_PBLOCK); ty >= 1; --ty) {
      if (!pair_geometry_ok(tx, ty)) continue;
      const long nt = (long)((n1 + tx - 1) / tx) * ((n2 + ty - 1) / ty);
      const long idle = nt * tx * ty - (long)n1 * n2;
      // on a tie, a tile the round-5 limits allowed (one position per thread, 512 / 468 / 384 LDS
      // slots) keeps its place: the measured choices there (n1 = 100: 20 x 34) stay as they were
      const int leg = (tx / 2 + 2) * (ty + 4) <= PFT_PBLOCK && 2 * PFT_PAIR_PADP + pair_lwp(tx) * (ty + 4) <= 512 &&
                      2 * PFT_PAIR_PADP + pair_lwp(tx) * (ty + 2) <= 468 && (tx / 2) * ty <= 384;
      if (best == 0 || nt < best || (nt == best && (idle < best_idle || (idle == best_idle && leg >= bleg)))) {
        best = nt;
        best_idle = idle;
        bx = tx;
        by = ty;
        bleg = leg;
      }
    }
  }
  *tx_out = bx;
  *ty_out = by;
  return best;
}

// gl's terms of a pair launch (its K's are the literal zeros of dgl, equation.c:731,874), each the
// reference's expression with those zeros (hybrid2.c:388/428, 408/449, 521, 667), so every gl
// value the kernel forms is the reference's bit for bit
static void pair_gl_consts(PairArgs& a, int first, double em2)
{
  volatile double z = 0.0;    // evaluated at run time, operation by operation, like the kernels
  const double k = z;
  if (first == 2) {
    a.glA = k * a.cinA;                                   // stage 2: K1 h/3 + x
    a.glB = (k + k) * a.cinB;                             // stage 3: (K1 + K2) h/6 + x
  } else {
    a.glA = (k + 3.0 * k) * a.cinA;                       // stage 4: (K1 + 3 K3) h/8 + x
    a.glB = (0.5 * k - 1.5 * k + 2.0 * k) * a.cinB;       // stage 5: (0.5 K1 - 1.5 K3 + 2 K4) h + x
  }
  a.glX = a.coef * (0.5 * (k + k) + 2.0 * k);             // x(t+h) = x + h/3 (0.5 (K1 + K5) + 2 K4)
  a.evgl = em2 * fabs(0.2 * k - 0.9 * k + 0.8 * k - 0.1 * k);   // the error-norm term
}

static int run_pair(pft_slab* s, int first, double t_a, double t_b, double h, double coef, int k_begin,
                    int k_end)
{
  const int mode = s->d.calc_mode;
  if (mode != 0 && mode != 1 && mode != 2 && mode != 10 && mode != 11) return -2;
  if (first != 2 && first != 4) return -2;
  PairArgs a;
  memset(&a, 0, sizeof(a));
  // the buffers' pointers minus one plane: the far ghost plane below the first field (pair_load)
  a.x = s->buf[PFT_BUF_X] - s->plane;
  a.k1 = s->buf[PFT_BUF_K1] - s->plane;
  a.k3 = s->buf[PFT_BUF_K3] - s->plane;
  a.out = (first == 2 ? s->buf[PFT_BUF_K3] : s->buf[PFT_BUF_XN]) - s->plane;
  a.noise = s->noise;
  a.eps_bits = s->scratch;
  a.nonfinite = (unsigned int*)(s->scratch + 1);
  a.fs = s->fs;
  a.n1 = s->d.n1;
  a.n2 = s->d.n2;
  a.n3 = s->d.n3;
  a.plane = s->plane;
  a.has_below = s->d.has_below;
  a.has_above = s->d.has_above;
  a.tx = s->pair_tx;
  a.ty = s->pair_ty;
  if (s->pair_ntile <= 0 || !pair_geometry_ok(a.tx, a.ty)) return -2;
  a.ntx = (a.n1 + a.tx - 1) / a.tx;
  a.ntile = a.ntx * ((a.n2 + a.ty - 1) / a.ty);
  // z-chunks by run_stage's cost model: a chunk of kz planes evaluates stage A on kz + 2 and loads
  // kz + 3; `occ` workgroups per CU (one: 141 KiB of LDS).  The boundary launch is the two-plane one.
  pft_zplan p;
  const int prc = slab_plan(s, &p, KZ_PAIR + (first == 4 ? 1 : 0), k_begin, k_end, a.ntile, pair_occupancy(first, mode), 2,
                            s->bdone != nullptr);
  if (prc <= 0) return prc;
  const bool bnd = p.bnd != 0, inl = p.inl != 0;
  plan_apply(s, first + 1, p, a);
  a.shards = s->eps_shards + (bnd ? PFT_EPS_SHARDS : 0);
  const long nwg = (long)a.nbw + (long)a.nint;   // the launch's workgroups
  a.T_topA = t_a < s->c.phase_switch_time ? s->c.top_temp1 : s->c.top_temp2;
  a.T_topB = t_b < s->c.phase_switch_time ? s->c.top_temp1 : s->c.top_temp2;
  a.cinA = pft_stepctl_stage(first, 0.0, h).cin;   // run_stage's stage-input coefficients
  a.cinB = pft_stepctl_stage(first + 1, 0.0, h).cin;
  a.coef = coef;
  a.em0 = s->d.eps_mult[0];
  a.em1 = s->d.eps_mult[1];
  pair_gl_consts(a, first, s->d.eps_mult[2]);
  // gl's inputs are x itself (GLX): gl_static, or gl_keep with finite coefficients, where
  // glA + x == glB + x == x + glX == x for every gl value of x (no -0.0, no NaN: gl_clean)
  const bool glx = s->d.gl_static ||
                   (s->gl_keep && std::isfinite(a.cinA) && std::isfinite(a.cinB) && std::isfinite(coef));
  a.gl_keep = glx ? 1 : 0;
  s->pub_armed = 0;
  const int split_pub = s->split_pub;
  s->split_pub = 0;
  if (first == 4 && s->inkernel_pub && !bnd && ((p.k_begin == 0 && p.k_end == s->d.n3) || inl)) {
    if (int rc = pub_arm(s, nwg, &a.part)) return rc;
    s->pub_armed = 1;
    s->pub_slot = s->defer_slot;
  } else if (first == 4 && s->inkernel_pub && bnd) {
    // split stage 4+5 (boundary, then interior: rk_solver do_pair): the boundary launch's partials
    // first, the interior's after them (the capacity for both now: no reallocation between the two
    // launches), reduced and published by the next stage-1 launch as for one launch
    if (int rc = pub_arm(s, (long)a.ntile * a.nchunk, &a.part, (long)a.ntile * (a.nchunk + s->d.n3))) return rc;
    s->split_pub = 1;
  } else if (first == 4 && split_pub && !bnd && s->defer_n > 0 &&
             s->defer_n + (long)a.ntile * a.nchunk <= s->part_cap) {
    a.part = s->part + 2 * (long)s->defer_n;
    s->defer_n += a.ntile * a.nchunk;
    s->pub_armed = 1;
    s->pub_slot = s->defer_slot;
  }
  if (first == 4) s->launch_part = a.part != nullptr;
  const dim3 g((unsigned)nwg);
  // bnd_mode 1, 2: the boundary launch beside the interior one.  On a 400 x 400 plane the interior
  // holds one workgroup per tile column, 220 of 256 CUs: the boundary's workgroups take the CUs it
  // leaves and the copies start while the interior still runs.  An interior launch of more
  // workgroups than CUs (several rounds, the 318^2 and 252^2 planes) leaves CUs only in its last
  // round, and beside is still no slower there than before (profiles/r05_ce_shapes.txt).  (Not so
  // a stage launch's boundary, whose interior fills the chip: run_stage, mode 1 only)
  const bool beside = bnd && s->bnd_mode != 0;
  const int lwp = pair_lwp(a.tx);
  return launch_planned(s, p, beside, [&](hipStream_t st) { launch_pair(first, mode, glx, lwp, g, st, a, s->c); });
}

extern "C" {

int pft_slab_set_pair(pft_slab* s, int on)
{
  if (on < 0 || on > 2) return -2;
  if (!s->pair_env) s->pair_on = on;
  return 0;
}

int pft_slab_pair_ok(const pft_slab* s)
{
  // automatic: slabs of at least PFT_PAIR_MIN_CELLS_PER_CU cells per CU.  Measured (A/B, one box):
  // 400^3 +28% (round 3), 200^3 (2 M cells, 7.8 Ki per CU) +6% since the 12-pair row pitch of
  // 100-wide planes (round 4: 14 384 against 13 575 Mcells*steps/s), 100^3 -28% (one workgroup
  // per CU marching 3-5 planes, two of them stage-A-only, against one plane per workgroup)
  if (s->pair_on == 1 && (double)s->plane * s->d.n3 < (double)s->n_cu * PFT_PAIR_MIN_CELLS_PER_CU) return 0;
  // z-neighbours: the two-plane halo (pft_comm_halo_deep) needs n3 >= 2, and stage A on a ghost
  // plane would need the neighbour's u_noise there (not exchanged: one launch per stage then)
  const bool nb = s->d.has_below || s->d.has_above;
  if (nb && (s->d.n3 < 2 || s->noise)) return 0;
  // (merson_pair addresses a field with 32-bit byte offsets; the limit is the one the round-6 LDS
  // DMA set, the three fields of a buffer from one base: 3 fields < 4 GiB, 178 M cells per slab)
  return s->pair_on && slab_kind(s) == KFUSED &&
         3.0 * (double)s->fs * 8.0 < 4294967296.0 && s->pair_ntile > 0;
}

int pft_slab_pair_geometry(const pft_slab* s, int* tx, int* ty)
{
  *tx = s->pair_tx;
  *ty = s->pair_ty;
  return s->pair_ntile > 0 ? 0 : -2;
}

int pft_slab_pair(pft_slab* s, int first, double t_a, double t_b, double h, double coef)
{
  return pft_slab_pair_range(s, first, t_a, t_b, h, coef, -1, -1);
}

int pft_slab_boundary_inline(const pft_slab* s)
{
  return s->bnd_mode >= 4 && s->bdone && s->d.n3 >= 5 && slab_kind(s) == KFUSED
             ? (s->bnd_mode == 5 ? PFT_K_ENDS_FIRST : PFT_K_INLINE)
             : 0;
}

int pft_slab_stage_inline(const pft_slab* s) { return s->stage_inline ? pft_slab_boundary_inline(s) : 0; }

int pft_slab_pair_inline(const pft_slab* s, int first)
{
  const int m = pft_slab_boundary_inline(s);
  if (!m) return 0;
  // A/B: PFT_CE_BND23 / PFT_CE_BND45 = 4 or 5 overrides the placement of one pair kernel
  const char* e = getenv(first == 2 ? "PFT_CE_BND23" : "PFT_CE_BND45");
  if (e && atoi(e) == 4) return PFT_K_INLINE;
  if (e && atoi(e) == 5) return PFT_K_ENDS_FIRST;
  // placement 5: end chunks first where the one-wave trigger kernel fits on a CU beside the pair
  // kernel's workgroup (pair 2+3: 216-221 VGPRs, 126 KiB of LDS).  Pair 4+5 at 256 VGPRs (every
  // calc mode but 2, scripts/kernel_resources.py) fills each SIMD's register file, so the trigger
  // holds a CU of its own for as long as it waits -- half the launch with end chunks, and one CU
  // fewer in one XCD costs that XCD a round of workgroups (400 x 400 x 100: 125 per XCD, 4 rounds
  // on 32 CUs, 5 on 31; pair 4+5 0.479 against 0.404 ms, profiles/r06_ce_inline.txt).  There the
  // two-plane boundary chunks (placement 4) free CUs within a few plane steps and the trigger ends
  // with them.
  if (m == PFT_K_ENDS_FIRST && first == 4 && s->d.calc_mode != 2) return PFT_K_INLINE;
  return m;
}

int pft_slab_pair_range(pft_slab* s, int first, double t_a, double t_b, double h, double coef, int k_begin,
                        int k_end)
{
  if (!pft_slab_pair_ok(s)) return -2;
  return run_pair(s, first, t_a, t_b, h, coef, k_begin, k_end);
}

int pft_slab_swap_buffers(pft_slab* s, int a, int b)
{
  if (a < 0 || a >= PFT_BUF_COUNT || b < 0 || b >= PFT_BUF_COUNT) return -2;
  double* t = s->buf[a];
  s->buf[a] = s->buf[b];
  s->buf[b] = t;
  const int p = s->phys[a];
  s->phys[a] = s->phys[b];
  s->phys[b] = p;
  return 0;
}

int pft_slab_accept(pft_slab* s) { return pft_slab_swap_buffers(s, PFT_BUF_X, PFT_BUF_XN); }

int pft_flat_alloc(double** p, size_t n)
{
  HIPCHK(hipMalloc((void**)p, n * sizeof(double)));
  return 0;
}
int pft_flat_free(double* p)
{
  if (p) HIPCHK(hipFree(p));
  return 0;
}
int pft_flat_h2d(double* dst, const double* src, size_t n, void* stream)
{
  HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream));
  return 0;
}
int pft_flat_d2h(double* dst, const double* src, size_t n, void* stream)
{
  HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream));
  return 0;
}
int pft_flat_combine(int stage, int n_chunks, const int* d_start, const int* d_size, const double* d_mult,
                     double coef, double h, const double* x, const double* k1, const double* k2, const double* k3,
                     const double* k4, const double* k5, double* out, double* d_eps2, void* stream)
{
  const int blocks = n_chunks < 4096 ? n_chunks : 4096;
  if (blocks <= 0) return -2;
  flat_combine_kernel<<<blocks, PFT_BLOCK, 0, (hipStream_t)stream>>>(
      stage, n_chunks, d_start, d_size, d_mult, coef, h, x, k1, k2, k3, k4, k5, out,
      (unsigned long long*)d_eps2, (unsigned int*)(d_eps2 + 1));
  HIPCHK(hipGetLastError());
  return 0;
}
int pft_stream_sync(void* stream)
{
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}
int pft_probe_copy(double* dst, const double* src, size_t n, void* stream)
{
  probe_copy_kernel<<<4096, 256, 0, (hipStream_t)stream>>>(dst, src, (long)n);
  HIPCHK(hipGetLastError());
  return 0;
}

int pft_dev_alloc(void** p, size_t bytes)
{
  HIPCHK(hipMalloc(p, bytes));
  return 0;
}
int pft_dev_free(void* p)
{
  if (p) HIPCHK(hipFree(p));
  return 0;
}
int pft_h2d(void* dst, const void* src, size_t bytes, void* stream)
{
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return 0;
}
int pft_memcpy_d2d_async(void* dst, const void* src, size_t bytes, void* stream)
{
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}
int pft_event_record_wait(void* from_stream, void* to_stream)
{
  hipEvent_t e;
  HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(hipEventRecord(e, (hipStream_t)from_stream));
  HIPCHK(hipStreamWaitEvent((hipStream_t)to_stream, e, 0));
  HIPCHK(hipEventDestroy(e));
  return 0;
}

}  // extern "C"
