// pft_slab.h -- host-internal: what the translation units of the HIP side share.  The slab object
// (struct pft_slab), the error plumbing (g_err, fail, HIPCHK), the launch-size constants, the host
// helpers that cross files, and the dispatch from the runtime (stage, calc_mode, gl_static) to the
// kernels' template arguments.  The translation units over the C ABI of include/pft_hip.h:
//   pft_kernels.hip  the step kernels (merson_stage, merson_fused, merson_pair), the slab object's
//                    API, the pft_hip_* shim
//   pft_halo.hip     the halo exchange (ipc transport, copy engines, boundary stream, trigger kernel)
//   pft_ic.hip       the initial condition on the device (f1)
//   pft_reduce.hip  diagnostics, exact means, formula diagnostics and histograms (f5, f6, f12, f13)
//   pft_snap.hip     snapshots (f7), region snapshots (f11)
// No device code crosses files: nothing is device-linked.  Every .hip includes this header first.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pft_frontend.h"
#include "../../include/pft_hip.h"
#include "../../include/pft_io.h"
#include "pft_stepctl.h"

#pragma clang fp contract(off)

#define PFT_LOCAL __attribute__((visibility("hidden")))   // crosses files, stays out of the library's exports

#define PFT_BLOCK 256      // threads per workgroup of the cache kernel (merson_stage)
#define PFT_FBLOCK 256     // ... of the fused stage kernel (merson_fused).  A/B: 512 (25 x 20-pair
                           // tiles, a third fewer halo loads) measured 3-5% slower at 400^3 -- one
                           // workgroup per CU where 256 fit two to four
#define PFT_TRING 8
#define PFT_PUB_SLOTS 64

// the thread's last error text (pft_hip_last_error): one definition, in pft_kernels.hip
extern PFT_LOCAL __thread char g_err[256];
PFT_LOCAL int fail(hipError_t e, const char* what);
#define HIPCHK(x)                                  \
  do {                                             \
    hipError_t e_ = (x);                           \
    if (e_ != hipSuccess) return fail(e_, #x);     \
  } while (0)

#define PFT_GATE_SLOTS 64

// a z-neighbour's buffers mapped into this process (ipc transport): the put kernel and the fused
// stage kernels store this slab's boundary planes straight into the neighbour's ghost plane
struct SlabPeer {
  int on;                              // 1: a neighbour on this side receives our boundary planes
  int opened;                          // 1: base[] / sig came from hipIpcOpenMemHandle (close them)
  double* base[PFT_BUF_COUNT];         // the neighbour's buffers by physical index
  unsigned long long* sig;             // the neighbour's flag words
  long fs;                             // its field stride
  int n3;                              // its interior planes
  int remote;                          // 1: on another GPU (xGMI)
  int staged;                          // 1: our planes go to its receive buffer (remote, or PFT_IPC_STAGED)
  double* rbuf;                        // its receive buffer
};

struct EpsShard;   // pft_kernels.hip

struct pft_slab {
  pft_slab_desc d;
  pft_consts c;          // (ralpha: slab_div_consts)
  double da_alpha, da_r; // the alpha it was computed for, and the value
  int da_valid;
  long fs;
  int plane;
  double* buf[PFT_BUF_COUNT];
  double* buf0[PFT_BUF_COUNT];   // the allocations by physical index (buf[] is permuted by swaps)
  int phys[PFT_BUF_COUNT];       // role -> physical index; every rank swaps identically, so a role
                                 // names the same physical buffer on every slab
  unsigned long long* sig;       // flag words written by the neighbours: [0] from below, [1] from
                                 // above (monotonic exchange sequence numbers); [8] put counter
  double* rbuf;                  // staged receive buffer (uncached, 2 x 12 planes; pft_slab_ipc_export)
  // copy-engine puts (pft_slab_halo_put_ce): the flags are raised by 8-byte SDMA copies from this
  // device table of sequence numbers (seq_base + 1 .. seq_base + PFT_SEQTAB), refilled from the
  // pinned halves seqhost[] when an exchange's number leaves it
  unsigned long long* seqtab;
  unsigned long long* seqhost;
  unsigned long long seq_base;
  int seq_half, seq_n;
  hipEvent_t ev_seq[2];  // recorded after each refill's H2D copy from that pinned half: the host
                         // rewrites a half only once the copy that read it last has run
  // the flags behind the completed plane copies (pft_slab_halo_put_ce, ce_fence): an event after
  // each copy stream's planes, waited for by the OTHER copy stream, which raises that side's flag
  int ce_fence;
  int gpu_ranks;         // ranks of the communicator on this slab's GPU (ipc attach; 0/1: alone)
  hipEvent_t ev_planes[2];
  // boundary launches on their own stream (pft_slab_set_boundary_stream; the copy-engine exchange):
  // a launch of the boundary planes (PFT_K_BOUNDARY/2) runs on `bnd` beside the interior launch on
  // the compute stream instead of before it; the exchange waits for ev_bnd, and so does the compute
  // stream before the next launch (pft_slab_halo_wait).  bnd_mode 1: every boundary launch, 2: the
  // pair kernels' (run_pair), 3: the pair kernels', with the halo waits on `bnd` (the boundary pipeline)
  int bnd_mode, bnd_pending, ce_streams;
  int ce_marked;         // pft_slab_halo_mark recorded ev_order[0] after the launch the next put_ce sends
  int bnd_split;         // the exchange's boundary launch ran before its interior on the compute stream
  int wait_streamops;    // A/B: halo waits as hipStreamWaitValue64 (env PFT_WAIT_STREAMOPS=1)
  hipStream_t bnd;
  hipEvent_t ev_bnd, ev_pre, ev_copy, ev_side, ev_join;
  // bnd_mode 4 (inline boundary): the pair kernels' boundary chunks lead their interior launch
  // (PFT_K_INLINE); its boundary workgroups count themselves in *bdone, and the exchange's copies
  // wait behind bnd_trigger_kernel for the count bdone_target (inline_pending: not yet sent)
  unsigned long long* bdone;
  unsigned long long bdone_target;
  int inline_pending;
  int trig_early;        // A/B (PFT_CE_TRIG): 1 the trigger queued with the launch, 0 with the copies
  int stage_inline;      // A/B (PFT_CE_STAGE_INLINE): stage launches inline too (else boundary first)
  hipEvent_t ev_trig;
  int put_role, put_f0, put_f1, put_deep;   // the exchange the last halo_put2 sent (its wait receives it)
  SlabPeer peer[2];              // [0] the neighbour below, [1] above
  int drop_puts;                 // fault injection: halo puts and flag raises skipped (PFT_IPC_DROP_PUTS)
  int ipc_poisoned;              // an ipc wait timed out: the flag words were forced past every
                                 // sequence number, so no later halo wait would block -- every halo
                                 // exchange, wait and sync refuses (PFT_ERR_IPC_TIMEOUT) until
                                 // pft_slab_ipc_close resets the flags (a detach / re-attach);
                                 // 2: the watched communicator aborted (PFT_ERR_COMM_ABORTED, for good)
  double* staging;      // host padded layout on the device (for upload/download)
  long S;                // host padded block (one field)
  unsigned long long* scratch;  // [0] eps bits, [1] nonfinite flag
  unsigned long long* host_scratch;  // pinned
  unsigned long long* host_pub;      // pinned, coherent: written by publish_kernel
  unsigned long long* host_pub_dev;  // its device address
  hipStream_t stream, comm;
  hipStream_t side;      // error-norm read-back while the compute stream runs ahead
  hipEvent_t ev_order[3];  // stream-order events: [0] compute -> comm, [1] comm -> compute,
                           // [2] the last boundary launch on the comm stream
  hipEvent_t ev_eps;     // recorded on the compute stream after the error norm is final
  int eps_marked;        // 1: publish kernel + event; 2: published by stage 5 itself (pub ring)
  // in-kernel publication (pft_slab_set_inkernel_publish): ring of 2-word slots in pinned,
  // coherent host memory, one per stage-5 launch; the host pre-sets a slot to the sentinel and
  // polls it after the launch
  int inkernel_pub;
  unsigned long long* pub_ring;      // host address (PFT_PUB_SLOTS x 2 words)
  unsigned long long* pub_ring_dev;  // its device address
  unsigned int* pub_count;           // device: finished workgroups of the publishing launch
  EpsShard* eps_shards;              // device: the error norm's shards (after pub_count's line)
  unsigned long long* part;          // device: deferred publication partials (2 words per workgroup)
  long part_cap;                     // ... their capacity in workgroups
  int defer_n;                       // workgroups of the armed error-norm launch awaiting reduction
  int defer_slot;                    // ... and its host slot
  int split_pub;                     // a split stage 4+5's boundary launch armed it; the interior follows
  // host-side memos (a small slab is host-bound: ~5 launches of a few us per attempted step)
  int fgeo_valid, fgeo_wx, fgeo_ty;  // fused_geometry(n1, n2) of this slab
  double fgeo_eff;
  struct KzMemo {                    // z-chunk cost model memo (chunk_kz): key (its arguments) -> kz,
    long key;                        // per launcher (KZ_*) and chunking rule (plain, ends-first)
    int kz;
  } kz_memo[14][2];
  int launch_nwg[6], launch_kz[6], launch_ntile[6];   // the last launch that ended stage 1..5 (pft_slab_launch_geometry)
  int launch_bnd[6];                 // ... and whether it was the boundary launch of a split stage
  int launch_part;                   // ... and whether the last error-norm launch stored deferred partials
  long pub_next;                     // slots used so far
  int pub_armed;                     // the last stage-5 launch publishes into slot pub_slot
  int pub_slot;
  // gated steps (f4, pft_slab_gate_*): the host's decisions on the next step go to a ring of
  // pinned slots (4 words: seq, t bits, h bits, pad); the speculative stage 1's extra workgroup
  // copies its slot into the device ring, which the pre-enqueued launches of that step read
  unsigned long long* gate_pin;      // host address, PFT_GATE_SLOTS x 4 words
  unsigned long long* gate_pin_dev;  // its device address
  unsigned long long* gate_dev;      // device ring, PFT_GATE_SLOTS x 4 words
  unsigned long long gate_seq;       // the last sequence number handed out
  unsigned long long gate_arm_seq;   // the next speculative stage-1 launch decides this step ...
  double gate_arm_t, gate_arm_h;     // ... (t, h) of it (ignored when that launch is gated itself)
  unsigned long long gate_use_seq;   // launches enqueued now are gated on this decision (0: not)
  pft_stepctl_consts gate_k;         // the solve's constants (pft_slab_gate_config)
  int gate_flip;         // test hook, env PFT_GATE_FLIP (StageArgs::d_flip)
  // eps-publication bookkeeping snapshots (pft_slab_book_save/load): the launches of the next
  // step are enqueued between this step's launches and the read of its error norm
  struct Book {
    long pub_next;
    int pub_armed, pub_slot, eps_marked, defer_n, defer_slot;
  } book[2];
  int kz;                // planes per workgroup z-march; 0 = automatic (z-chunk cost model)
  int n_cu;               // compute units of the slab's device
  int cu_reserved;        // of them kept off the compute stream for the boundary launches (CU mask)
  double* noise;         // device u_noise (n3*plane) or null
  int tile_wx;           // 32 / 16: LDS-tiled kernels with that many pairs per row; 1: automatic;
                         // 2: LDS-tiled at any size, automatic tile; 0: cache-based
  int n1_tiled_ok;
  int recompute;         // 1: stage inputs rebuilt from x and the K's (no aux arrays)
  int gl_keep;           // X and XN hold the same gl, and x + c*0.0 == x for every gl value
  int pair_on;           // pair kernels (merson_pair): 0 off, 1 automatic (large slabs), 2 wherever
                         // they fit (pft_slab_set_pair); env PFT_PAIR overrides
  int pair_env;          // PFT_PAIR was set
  int pair_tx, pair_ty;  // pair tile (pair_geometry, once per slab); 0 x 0: none fits
  long pair_ntile;
  // f5 diagnostics (pft_slab_diag): device accumulators (PFT_DIAG_HEAD words, then one ice count
  // per interior plane) and their pinned host copy, allocated by the first call
  unsigned long long* diag_dev;
  unsigned long long* diag_host;     // pinned
  int diag_wgs;          // cap on the reduction's workgroups; 0: 8 per CU (env PFT_DIAG_WGS: A/B, tests)
  int diag_timing;       // 1: HIP events around the kernel (pft_slab_diag_timing)
  hipEvent_t ev_diag[2];
  // f6 means (pft_slab_means): the slab's record, then one record per interior plane, and their
  // pinned host copy, allocated by the first call; events around the kernel pair
  unsigned long long* means_dev;
  unsigned long long* means_host;    // pinned
  int means_timing;
  hipEvent_t ev_means[2];
  // f12 formula diagnostics (pft_slab_formulas): PFT_FORMULA_MAX total records, then n3 plane
  // records per program, and their pinned host copy, allocated by the first call; the programs
  // and their tables as one blob (device and pinned host, grown on demand); events around the
  // kernel pair
  unsigned long long* formula_dev;
  unsigned long long* formula_host;  // pinned
  char* formula_prog_dev;
  char* formula_prog_host;           // pinned
  size_t formula_prog_cap;
  int formula_timing;
  hipEvent_t ev_formula[2];
  // f13 histograms (pft_slab_hist): the slab's row of 4 + nbins words, then one row per interior
  // plane, and their pinned host copy, grown on demand (hist_cap bytes each); the programs and the
  // edges travel in the f12 blob; events around the kernel pair
  unsigned long long* hist_dev;
  unsigned long long* hist_host;     // pinned
  size_t hist_cap;
  int hist_timing;
  hipEvent_t ev_hist[2];
  // f15 maps (pft_slab_map): 7 accumulator words per pixel and their pinned host copy, grown on
  // demand (map_cap bytes each); the programs travel in the f12 blob; events around the kernel
  unsigned long long* map_dev;
  unsigned long long* map_host;      // pinned
  size_t map_cap;
  int map_timing;
  hipEvent_t ev_map[2];
  // f7 snapshots (pft_slab_snapshot_export / pft_slab_image): the image-sized pinned, host-mapped
  // buffer the background writer reads (allocated by the first call, freed at destroy once the
  // writer is done with it), the device staging image of the staged host link, events around the
  // export kernel
  void* snap_host;
  void* snap_host_dev;   // its device address
  void* snap_stage;
  int snap_timing;
  hipEvent_t ev_snap[2];
  int region_wgs;        // f11: cap on region_kernel's workgroups; 0: 8 per CU (env PFT_REGION_WGS: tests)
  double timeout_s;    // bound on a host wait for the compute stream while ipc peers are on
                         // (env PFT_IPC_TIMEOUT, default 300 s; slab_wait)
  pft_slab_watch_fn watch;   // communicator watchdog (RCCL: async error / expiry -> abort)
  void* watch_ctx;
  double watch_timeout_s;
  // per-stage timing: a ring of begin/end event pairs, so that kernels still running when the
  // host collects (the speculative stage 1) are picked up by a later collect
  hipEvent_t tev[6][PFT_TRING][2];
  int thead[6], ttail[6];      // next slot to record / oldest slot not yet collected
  double tacc_ms[6];           // collected but not yet handed out
  long tacc_n[6];
};

// kernel flavours: KCACHE (any n1, aux arrays), KFUSED (LDS tile, stage inputs recomputed from x
// and the K's -- the default for even n1); 1 was the retired LDS-tiled aux-array kernel
enum { KCACHE = 0, KFUSED = 2 };

// host helpers that cross files, each commented at its definition
PFT_LOCAL int slab_poisoned(pft_slab* s, const char* what);              // pft_kernels.hip
PFT_LOCAL int slab_wait(pft_slab* s, hipEvent_t ev, const char* what);
PFT_LOCAL void slab_trigger(pft_slab* s);                                // pft_halo.hip

// The runtime (stage, calc_mode, flag) to template arguments: f is a generic lambda, called with the
// value as a std::integral_constant, so each call site names its kernel once and the compiler
// instantiates it for every value (no table, no indirect call).  The callers checked the value.
// HIP events around a family's kernels (diag, means, formulas, hist, snapshot): its pft_slab_*_timing
// entry switches them on (the events are made at the first use), its pft_slab_*_last_ms reads the
// last call's time; flag and ev name the family's own fields
static inline int slab_timing_set(pft_slab* s, int pft_slab::*flag, hipEvent_t (pft_slab::*ev)[2], int on)
{
  if (!s) return -2;
  for (int i = 0; i < 2 && on; ++i)
    if (!(s->*ev)[i]) HIPCHK(hipEventCreate(&(s->*ev)[i]));
  s->*flag = on ? 1 : 0;
  return 0;
}

static inline int slab_timing_ms(pft_slab* s, int pft_slab::*flag, hipEvent_t (pft_slab::*ev)[2], double* ms)
{
  if (!s || !ms || !(s->*flag)) return -2;
  float f = 0.0f;
  HIPCHK(hipEventElapsedTime(&f, (s->*ev)[0], (s->*ev)[1]));
  *ms = f;
  return 0;
}

template <int N>
using pft_int = std::integral_constant<int, N>;

template <class F>
static inline decltype(auto) with_mode(int mode, F&& f)
{
  switch (mode) {
    case 0: return f(pft_int<0>{});
    case 1: return f(pft_int<1>{});
    case 2: return f(pft_int<2>{});
    case 10: return f(pft_int<10>{});
    default: return f(pft_int<11>{});
  }
}

template <class F>
static inline decltype(auto) with_stage(int stage, F&& f)
{
  switch (stage) {
    case 0: return f(pft_int<0>{});
    case 1: return f(pft_int<1>{});
    case 2: return f(pft_int<2>{});
    case 3: return f(pft_int<3>{});
    case 4: return f(pft_int<4>{});
    default: return f(pft_int<5>{});
  }
}

template <class F>
static inline decltype(auto) with_bool(bool b, F&& f)
{
  if (b) return f(std::true_type{});
  return f(std::false_type{});
}
