// pft_halo.hip -- the halo exchange of the ipc transport: the put / receive / wait / signal kernels,
// the copy-engine exchange with its sequence table and its trigger kernel (inline boundaries), the
// ipc export, peer and close entries, the boundary stream, and every pft_slab_halo_* entry.
#include "pft_slab.h"

// the copy-engine exchange of an inline boundary (PFT_K_INLINE): this one-wave kernel ends once the
// boundary workgroups of the launch have counted themselves (*bdone >= target, monotonic), so the
// plane copies queued behind it on the comm stream start while that launch's interior still runs.
// It sits on a CU the boundary workgroups freed; nothing it waits for depends on another rank.
__global__ __launch_bounds__(64) void bnd_trigger_kernel(const unsigned long long* bdone, unsigned long long target)
{
  if (threadIdx.x == 0)
    while (__hip_atomic_load(bdone, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target) __builtin_amdgcn_s_sleep(2);
}

// the trigger on the comm stream, behind a launch with an inline boundary (launch_planned,
// pft_kernels.hip, which checks the launch)
void slab_trigger(pft_slab* s) { bnd_trigger_kernel<<<1, 64, 0, s->comm>>>(s->bdone, s->bdone_target); }

// ------------------------------------------------------------------------------------------
// ipc transport (pft_comm.h): this slab's boundary planes go straight into the z-neighbours' ghost
// planes (IPC-mapped device memory, on this GPU or over xGMI), then the last workgroup publishes the
// exchange's sequence number in the neighbours' flag words; each side's stream waits for its own
// flags (hipStreamWaitValue64), so the next stage starts only once both ghost planes are in.

struct PutArgs {
  const double* src;          // this slab's buffer (one role)
  long fs;
  int plane, n3, f0, nf;
  double* dlo;                // the neighbour below: its top ghost plane (n3' + 1) of field 0, or null
  long dlo_fs;
  double* dhi;                // the neighbour above: its bottom ghost plane (0) of field 0, or null
  long dhi_fs;
  int deep;                   // 1: also the second planes, into the neighbours' far ghost planes
  double* flo;                // the neighbour below's far plane above (n3' + 2) of field 0
  double* fhi;                // the neighbour above's far plane below (-1) of field 0
};

__global__ __launch_bounds__(256) void halo_put_kernel(PutArgs a)
{
  const long n = (long)a.nf * a.plane;   // doubles per side and depth
  const long tot = (a.deep ? 4 : 2) * n;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
    const int part = (int)(e / n);       // 0: plane 1 down, 1: plane n3 up, 2: plane 2 down (far), 3: plane n3-1 up (far)
    const long r = e - part * n;
    const int f = (int)(r / a.plane);
    const long c = r - (long)f * a.plane;
    const int q = a.f0 + f;
    if (part == 0) {
      if (a.dlo) a.dlo[q * a.dlo_fs + c] = a.src[q * a.fs + (long)a.plane + c];
    } else if (part == 1) {
      if (a.dhi) a.dhi[q * a.dhi_fs + c] = a.src[q * a.fs + (long)a.n3 * a.plane + c];
    } else if (part == 2) {
      if (a.flo) a.flo[q * a.dlo_fs + c] = a.src[q * a.fs + 2L * a.plane + c];
    } else {
      if (a.fhi) a.fhi[q * a.dhi_fs + c] = a.src[q * a.fs + (long)(a.n3 - 1) * a.plane + c];
    }
  }
}

// Staged receive (pft_slab_halo_wait): the planes the neighbours put into this slab's receive
// buffer rbuf (uncached; two slots by the exchange's parity, each [side][depth][field][plane], side
// 0 from below, 1 from above; depth 0 the ghost plane, 1 the far ghost plane) copied into the ghost planes of buffer dst, fields
// [f0, f0 + nf), for the sides in `sides` (bit 0 below, bit 1 above)
struct RecvArgs {
  const double* rbuf;
  double* dst;                // the buffer (pft_slab_buffer layout: plane 0 = ghost below)
  long fs;
  int plane, n3, f0, nf, depth, sides;
};

__global__ __launch_bounds__(256) void halo_recv_kernel(RecvArgs a)
{
  const long n = (long)a.nf * a.plane;
  const long tot = 4L * n;              // (side, depth) parts, skipped where not received
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
    const int part = (int)(e / n);
    const int side = part >> 1, depth = part & 1;
    if (!((a.sides >> side) & 1) || depth >= a.depth) continue;
    const long r = e - part * n;
    const int f = (int)(r / a.plane);
    const long c = r - (long)f * a.plane;
    const int q = a.f0 + f;
    const long pl = side == 0 ? (depth == 0 ? 0L : -1L) : (long)a.n3 + 1 + depth;
    a.dst[q * a.fs + pl * a.plane + c] = a.rbuf[((long)(side * 2 + depth) * 3 + q) * a.plane + c];
  }
}

// The receiving side of an exchange in ONE launch (pft_slab_halo_wait): thread 0 of every workgroup
// waits until both flag words reach seq (system-scope atomic loads of uncached memory: never served
// from a cache), then -- staged receive -- the workgroups copy the receive buffer into the ghost
// planes (halo_recv_kernel's loop).  It replaces hipStreamWaitValue64 per flag (the runtime runs each
// as a kernel of its own, ~3 us apiece) and the separate receive launch.  Every wave exits: the
// flags come from the neighbours, or from the slab itself when a wait times out (slab_timed_out
// releases them past every sequence number).
struct WaitArgs {
  const unsigned long long* f0;   // flag from below, or null
  const unsigned long long* f1;   // flag from above, or null
  unsigned long long seq;
  int recv;                       // 1: then copy r
  RecvArgs r;
};

__global__ __launch_bounds__(256) void halo_wait_kernel(WaitArgs a)
{
  if (threadIdx.x == 0) {
    if (a.f0)
      while (__hip_atomic_load(a.f0, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < a.seq) __builtin_amdgcn_s_sleep(2);
    if (a.f1)
      while (__hip_atomic_load(a.f1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < a.seq) __builtin_amdgcn_s_sleep(2);
  }
  __syncthreads();
  if (!a.recv) return;
  const RecvArgs& r = a.r;
  const long n = (long)r.nf * r.plane;
  const long tot = 4L * n;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
    const int part = (int)(e / n);
    const int side = part >> 1, depth = part & 1;
    if (!((r.sides >> side) & 1) || depth >= r.depth) continue;
    const long rr = e - part * n;
    const int f = (int)(rr / r.plane);
    const long c = rr - (long)f * r.plane;
    const int q = r.f0 + f;
    const long pl = side == 0 ? (depth == 0 ? 0L : -1L) : (long)r.n3 + 1 + depth;
    r.dst[q * r.fs + pl * r.plane + c] = r.rbuf[((long)(side * 2 + depth) * 3 + q) * r.plane + c];
  }
}

// raises the neighbours' flags once the kernels before it on the stream (the put, or a stage
// kernel that stored its boundary planes into the neighbours' ghost planes) have completed: their
// stores are released at kernel end; with a neighbour on another GPU a system-scope fence first
// (the flag must not overtake the plane over xGMI).  One thread, vector atomics only.
__global__ void halo_signal_kernel(unsigned long long* slo, unsigned long long* shi, unsigned long long seq,
                                   int remote)
{
  if (threadIdx.x != 0) return;
  if (remote) __threadfence_system();
  if (slo) __hip_atomic_store(slo, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (shi) __hip_atomic_store(shi, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

extern "C" {

static int ensure_rbuf(pft_slab* s)
{
  // two slots (exchange sequence number parity): a neighbour can be one exchange ahead -- its
  // next put needs only our flag of this exchange, which we raise before copying its planes out
  if (!s->rbuf) HIPCHK(hipExtMallocWithFlags((void**)&s->rbuf, sizeof(double) * 24 * (size_t)s->plane, hipDeviceMallocUncached));
  return 0;
}

int pft_slab_ipc_export(pft_slab* s, void* handles)
{
  hipIpcMemHandle_t* h = (hipIpcMemHandle_t*)handles;
  int rc = ensure_rbuf(s);
  if (rc) return rc;
  for (int b = 0; b < PFT_BUF_COUNT; ++b) HIPCHK(hipIpcGetMemHandle(&h[b], s->buf0[b]));
  HIPCHK(hipIpcGetMemHandle(&h[PFT_BUF_COUNT], s->sig));
  HIPCHK(hipIpcGetMemHandle(&h[PFT_BUF_COUNT + 1], s->rbuf));
  return 0;
}

int pft_ipc_staged_env(void)
{
  const char* e = getenv("PFT_IPC_STAGED");
  return e && atoi(e) == 1;
}

int pft_slab_ipc_set_peer(pft_slab* s, int side, const void* handles, int n3, long fs, int remote,
                          int peer_staged)
{
  if (side < 0 || side > 1) return -2;
  SlabPeer& p = s->peer[side];
  if (p.on) return -2;                  // pft_slab_ipc_close first
  if (!handles) {
    // self exchange (diagnostic, one slab): the planes land in the slab's own ghost planes, which a
    // single slab never reads (mirror bottom, Dirichlet top)
    int rc = ensure_rbuf(s);
    if (rc) return rc;
    for (int b = 0; b < PFT_BUF_COUNT; ++b) p.base[b] = s->buf0[b] + s->plane;
    p.sig = s->sig;
    p.rbuf = s->rbuf;
    p.staged = pft_ipc_staged_env();
    p.n3 = s->d.n3;
    p.fs = s->fs;
    p.opened = 0;
    p.on = 1;
    return 0;
  }
  const hipIpcMemHandle_t* h = (const hipIpcMemHandle_t*)handles;
  for (int b = 0; b <= PFT_BUF_COUNT + 1; ++b) {
    void* ptr = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&ptr, h[b], hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      for (int q = 0; q < b && q < PFT_BUF_COUNT; ++q) (void)hipIpcCloseMemHandle(p.base[q] - s->plane);
      if (b > PFT_BUF_COUNT) (void)hipIpcCloseMemHandle(p.sig);
      return fail(e, "hipIpcOpenMemHandle");
    }
    if (b < PFT_BUF_COUNT) p.base[b] = (double*)ptr + s->plane;   // the neighbour's buffer pointer
    else if (b == PFT_BUF_COUNT) p.sig = (unsigned long long*)ptr;
    else p.rbuf = (double*)ptr;
  }
  p.n3 = n3;
  p.fs = fs;
  p.remote = remote ? 1 : 0;   // the caller compared the GPUs' identities (pft_hip_device_ident)
  // A neighbour on another GPU writes into our receive buffer (uncached) rather than our ghost
  // planes, and we copy it in after the flag wait: no L2 of ours can hold a stale line of what it
  // wrote.  Both sides take the same decision: remote is symmetric, and the
  // env (the test hook that stages between processes on one GPU) counts if either side set it --
  // a sender putting into ghost planes that the receiver overwrites from its receive buffer, or
  // the other way round, would corrupt the halo without any error.
  p.staged = p.remote || pft_ipc_staged_env() || peer_staged;
  p.opened = 1;
  p.on = 1;
  return 0;
}

int pft_slab_ipc_close(pft_slab* s)
{
  if (s->ipc_poisoned == 1) {
    // the flags were forced past every sequence number: back to 0 for the next attach (the compute
    // stream has drained, slab_wait)
    (void)hipStreamSynchronize(s->stream);
    (void)hipStreamSynchronize(s->side);
    if (s->bnd) (void)hipStreamSynchronize(s->bnd);

    (void)hipStreamSynchronize(s->comm);
    HIPCHK(hipMemset(s->sig, 0, 2 * sizeof(unsigned long long)));
    HIPCHK(hipDeviceSynchronize());
    s->ipc_poisoned = 0;
  }
  if ((s->peer[0].on && s->peer[0].opened) || (s->peer[1].on && s->peer[1].opened)) {
    // the copy-engine exchange's streams write into the mappings about to be closed: drained first
    // (they wait only on compute-stream work, which the detach's pft_slab_sync has drained)
    if (s->comm) (void)hipStreamSynchronize(s->comm);
    if (s->side) (void)hipStreamSynchronize(s->side);
  }
  for (int side = 0; side < 2; ++side) {
    SlabPeer& p = s->peer[side];
    if (p.on && p.opened) {
      for (int b = 0; b < PFT_BUF_COUNT; ++b) (void)hipIpcCloseMemHandle(p.base[b] - s->plane);
      (void)hipIpcCloseMemHandle(p.sig);
      (void)hipIpcCloseMemHandle(p.rbuf);
    }
    memset(&p, 0, sizeof(p));
  }
  return 0;
}

int pft_slab_halo_put(pft_slab* s, int role, int f0, int f1, unsigned long long seq)
{
  return pft_slab_halo_put2(s, role, f0, f1, 0, seq);
}

double* pft_slab_far(pft_slab* s, int which, int q, int side)
{
  if (which < 0 || which >= PFT_BUF_COUNT || q < 0 || q > 2 || side < 0 || side > 1) return nullptr;
  return s->buf[which] + q * s->fs + (side ? (long)(s->d.n3 + 2) * s->plane : -(long)s->plane);
}

int pft_slab_halo_put2(pft_slab* s, int role, int f0, int f1, int deep, unsigned long long seq)
{
  if (role < 0 || role >= PFT_BUF_COUNT || f0 < 0 || f1 > 3 || f1 <= f0) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_halo_put2");
  s->put_role = role;
  s->put_f0 = f0;
  s->put_f1 = f1;
  s->put_deep = deep ? 1 : 0;
  if (s->drop_puts) return 0;
  const int ph = s->phys[role];
  PutArgs a;
  memset(&a, 0, sizeof(a));
  a.src = s->buf[role];
  a.fs = s->fs;
  a.plane = s->plane;
  a.n3 = s->d.n3;
  a.f0 = f0;
  a.nf = f1 - f0;
  // staged: into the neighbour's receive buffer [side][depth][field][plane] -- the neighbour below
  // receives our planes as "from above" (side 1), the one above as "from below" (side 0)
  const long P = s->plane;
  const long slot = (long)(seq & 1) * 12 * P;   // the receive-buffer slot of this exchange
  if (s->peer[0].on) {
    a.dlo = s->peer[0].staged ? s->peer[0].rbuf + slot + (1 * 2 + 0) * 3 * P : s->peer[0].base[ph] + (long)(s->peer[0].n3 + 1) * P;
    a.dlo_fs = s->peer[0].staged ? P : s->peer[0].fs;
  }
  if (s->peer[1].on) {
    a.dhi = s->peer[1].staged ? s->peer[1].rbuf + slot + (0 * 2 + 0) * 3 * P : s->peer[1].base[ph];
    a.dhi_fs = s->peer[1].staged ? P : s->peer[1].fs;
  }
  if (!a.dlo && !a.dhi) return 0;
  if (deep) {
    // the second boundary planes into the neighbours' far ghost planes (pft_slab_far layout)
    a.deep = 1;
    if (s->peer[0].on)
      a.flo = s->peer[0].staged ? s->peer[0].rbuf + slot + (1 * 2 + 1) * 3 * P : s->peer[0].base[ph] + (long)(s->peer[0].n3 + 2) * P;
    if (s->peer[1].on) a.fhi = s->peer[1].staged ? s->peer[1].rbuf + slot + (0 * 2 + 1) * 3 * P : s->peer[1].base[ph] - P;
  }
  const long n = (deep ? 4L : 2L) * a.nf * s->plane;
  const int blocks = (int)std::min<long>(1024, std::max<long>(1, (n + 255) / 256));
  halo_put_kernel<<<blocks, 256, 0, s->stream>>>(a);
  HIPCHK(hipGetLastError());
  return pft_slab_halo_signal(s, seq);
}

#define PFT_SEQTAB 4096

// The ipc exchange on the copy engines (SDMA): after the launch that wrote the boundary planes (an
// event on the compute stream), the comm stream copies them into the neighbours' ghost (and far
// ghost) planes -- or their receive buffers when staged -- with hipMemcpyDeviceToDeviceNoCU, then
// raises the neighbours' flags with 8-byte copies of the sequence number from seqtab.  No kernel:
// the copies need no CU, so they run beside the interior launch that holds every CU's LDS (a blit
// kernel, or RCCL's, waits for that launch to end: profiles/r05_sdma_probe.txt).  The receiver
// side is unchanged (pft_slab_halo_wait: the compute stream waits for the flags; staged: the
// receive kernel), so a sender may use either put.
int pft_slab_halo_put_ce(pft_slab* s, int role, int f0, int f1, int deep, unsigned long long seq)
{
  if (role < 0 || role >= PFT_BUF_COUNT || f0 < 0 || f1 > 3 || f1 <= f0 || seq == 0) return -2;
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_halo_put_ce");
  const int marked = s->ce_marked;
  s->ce_marked = 0;
  s->put_role = role;
  s->put_f0 = f0;
  s->put_f1 = f1;
  s->put_deep = deep ? 1 : 0;
  if (s->drop_puts) return 0;
  if (!s->peer[0].on && !s->peer[1].on) return 0;
  if (!s->seqtab) {
    HIPCHK(hipMalloc((void**)&s->seqtab, sizeof(unsigned long long) * PFT_SEQTAB));
    HIPCHK(hipHostMalloc((void**)&s->seqhost, 2 * sizeof(unsigned long long) * PFT_SEQTAB, hipHostMallocDefault));
    for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreateWithFlags(&s->ev_seq[i], hipEventDisableTiming));
    s->seq_base = ~0ULL;
    // test hook PFT_CE_SEQTAB=n (2..4096): a table of n numbers, refilled every n exchanges
    const char* et = getenv("PFT_CE_SEQTAB");
    s->seq_n = (et && atoi(et) >= 2 && atoi(et) <= PFT_SEQTAB) ? atoi(et) : PFT_SEQTAB;
    // the flags behind an explicit completion of the plane copies (default 1; PFT_CE_FENCE=0: each
    // flag copy right behind its planes on the same stream, relying on the in-order SDMA queue)
    const char* ef = getenv("PFT_CE_FENCE");
    s->ce_fence = !(ef && atoi(ef) == 0);
    for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreateWithFlags(&s->ev_planes[i], hipEventDisableTiming));
  }
  const int NSEQ = s->seq_n;
  if (s->seq_base == ~0ULL || seq <= s->seq_base || seq > s->seq_base + NSEQ) {
    // the next block of sequence numbers, from the pinned half not used by the previous refill
    s->seq_base = (seq - 1) / NSEQ * NSEQ;
    s->seq_half ^= 1;
    if (s->ce_streams != 1) {
      // the side stream's last flag copy reads the old table: the refill (comm stream) waits for it
      HIPCHK(hipEventRecord(s->ev_side, s->side));
      HIPCHK(hipStreamWaitEvent(s->comm, s->ev_side, 0));
    }
    // this pinned half was last read by the refill copy two refills ago: the host rewrites it only
    // once that copy has run (with a small table -- the PFT_CE_SEQTAB test hook -- the speculative
    // pipeline can hold that many exchanges queued)
    // (bounded like every host wait with ipc peers: a lost peer can hold that copy's stream)
    {
      const int wrc = slab_wait(s, s->ev_seq[s->seq_half], "pft_slab_halo_put_ce (seqtab refill)");
      if (wrc) return wrc;
    }
    unsigned long long* h = s->seqhost + (size_t)s->seq_half * PFT_SEQTAB;
    for (int i = 0; i < NSEQ; ++i) h[i] = s->seq_base + 1 + i;
    HIPCHK(hipMemcpyAsync(s->seqtab, h, sizeof(unsigned long long) * NSEQ, hipMemcpyHostToDevice, s->comm));
    HIPCHK(hipEventRecord(s->ev_seq[s->seq_half], s->comm));
    if (s->ce_streams != 1) {
      // the side stream's flag copies read the new table: this exchange's (and so every later one's)
      // follow the refill.  (An event on every exchange instead held each side flag behind the comm
      // stream's copies and put a marker between the comm stream's last copy and its flag: ~10-20
      // us later flags, profiles/r05_ce_trace_pipe.txt.)
      HIPCHK(hipEventRecord(s->ev_copy, s->comm));
      HIPCHK(hipStreamWaitEvent(s->side, s->ev_copy, 0));
    }
  }
  // the planes to the neighbour below go on the comm stream, to the one above on the side stream
  // (two copy engines; ce_streams = 1: all on the comm stream), each followed by its neighbour's
  // flag.  (Four streams, a side's copies alternating between two, measured slower: 11 300-12 600
  // against 16 000 Mcells*steps/s on the 800^3 rank slab, profiles/r05_ce_ab.txt; removed.)
  hipStream_t cs[2] = {s->comm, s->ce_streams == 1 ? s->comm : s->side};
  if (s->inline_pending) {
    // inline boundary: the copies start once the launch's boundary workgroups have counted
    // themselves -- not at its end, and with no event on the compute stream between them
    // (trig_early: the trigger is on the comm stream already, queued with the launch)
    s->inline_pending = 0;
    if (!s->trig_early) {
      bnd_trigger_kernel<<<1, 64, 0, cs[0]>>>(s->bdone, s->bdone_target);
      HIPCHK(hipGetLastError());
    }
    if (cs[1] != cs[0]) {
      HIPCHK(hipEventRecord(s->ev_trig, cs[0]));
      HIPCHK(hipStreamWaitEvent(cs[1], s->ev_trig, 0));
    }
  } else {
    hipEvent_t ready = s->bnd_pending ? s->ev_bnd : s->ev_order[0];
    if (!s->bnd_pending && !marked) HIPCHK(hipEventRecord(s->ev_order[0], s->stream));
    HIPCHK(hipStreamWaitEvent(cs[0], ready, 0));
    if (cs[1] != cs[0]) HIPCHK(hipStreamWaitEvent(cs[1], ready, 0));
  }
  const int ph = s->phys[role];
  const long P = s->plane, n3 = s->d.n3;
  const long slot = (long)(seq & 1) * 12 * P;
  const size_t pb = sizeof(double) * (size_t)P;
  for (int side = 0; side < 2; ++side) {
    const SlabPeer& p = s->peer[side];
    if (!p.on) continue;
    for (int q = f0; q < f1; ++q) {
      const double* src = s->buf[role] + q * s->fs;
      if (!p.staged) {
        // below: our planes 1 (, 2) into its ghost n3'+1 (, far n3'+2); above: our planes (n3-1,) n3
        // into its (far -1,) ghost 0 -- contiguous on both ends
        double* dst = side == 0 ? p.base[ph] + q * p.fs + (p.n3 + 1) * P : p.base[ph] + q * p.fs - (deep ? P : 0);
        const double* sp = side == 0 ? src + P : src + (deep ? n3 - 1 : n3) * P;
        HIPCHK(hipMemcpyAsync(dst, sp, (deep ? 2 : 1) * pb, hipMemcpyDeviceToDeviceNoCU, cs[side]));
      } else {
        // its receive buffer [slot][side][depth][field][plane]: the neighbour below receives our
        // planes as "from above" (side 1), the one above as "from below" (side 0)
        for (int d = 0; d < (deep ? 2 : 1); ++d) {
          double* dst = p.rbuf + slot + ((long)((side == 0 ? 1 : 0) * 2 + d) * 3 + q) * P;
          const double* sp = side == 0 ? src + (1 + d) * P : src + (n3 - d) * P;
          HIPCHK(hipMemcpyAsync(dst, sp, pb, hipMemcpyDeviceToDeviceNoCU, cs[side]));
        }
      }
    }
  }
  const unsigned long long* sv = s->seqtab + (seq - 1 - s->seq_base);
  // The neighbour reads the planes once it sees the flag, so the flag must not land before them.
  // ce_fence (default): the flag copy goes on a stream of its own behind an event recorded after
  // the side's plane copies.  The runtime turns that event wait into a dependency on the copies'
  // completion signal (hsa_amd_memory_async_copy, hsa_ext_amd.h: "the copy will start after every
  // [dependent] signal has been observed with the value 0", and the completion signal is
  // decremented "when the copy operation is finished"), so the flag copy starts only after the
  // plane copies have finished -- an ordering the HSA interface states, where a flag copy right
  // behind them on the same stream relies on the SDMA queue retiring its writes in order (not a
  // documented property across xGMI; PFT_CE_FENCE=0 restores that form for A/B).  The receiver's
  // side is the system-scope acquire load of the flag in halo_wait_kernel (hsa_ext_amd.h asks the
  // receiving device for a system-scope acquire before it uses a copy's destination).
  // No stream is added for it: a process has 4 hardware queues (GPU_MAX_HW_QUEUES) and already 4
  // streams (compute, boundary, comm, side); a fifth and sixth share queues with them, and their
  // waits then hold up unrelated work -- one flag stream per side measured that way (DESIGN
  // section 6).  So each side's flag goes on the OTHER copy stream, behind an event after this
  // side's planes: with two neighbours both flags land after both sides' planes (the two run side
  // by side, of equal size), each ordered after its own planes by the event.  With one copy stream
  // (ce_streams 1) the stream order is all there is.
  hipStream_t fs[2] = {cs[0], cs[1]};
  if (s->ce_fence && cs[1] != cs[0]) {
    for (int side = 0; side < 2; ++side)
      if (s->peer[side].on) HIPCHK(hipEventRecord(s->ev_planes[side], cs[side]));
    for (int side = 0; side < 2; ++side)
      if (s->peer[side].on) {
        fs[side] = cs[1 - side];
        HIPCHK(hipStreamWaitEvent(fs[side], s->ev_planes[side], 0));
      }
  }
  if (s->peer[0].on) HIPCHK(hipMemcpyAsync(s->peer[0].sig + 1, sv, 8, hipMemcpyDeviceToDeviceNoCU, fs[0]));
  if (s->peer[1].on) HIPCHK(hipMemcpyAsync(s->peer[1].sig + 0, sv, 8, hipMemcpyDeviceToDeviceNoCU, fs[1]));
  return 0;
}

int pft_slab_halo_mark(pft_slab* s)
{
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_halo_mark");
  if (!s->bnd_pending && !s->inline_pending) HIPCHK(hipEventRecord(s->ev_order[0], s->stream));
  s->ce_marked = 1;
  return 0;
}

int pft_slab_set_boundary_stream(pft_slab* s, int on)
{
  if (on && !s->bnd) {
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(hipStreamCreateWithPriority(&s->bnd, hipStreamNonBlocking, hi));
    HIPCHK(hipEventCreateWithFlags(&s->ev_bnd, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s->ev_pre, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s->ev_copy, hipEventDisableTiming));
  }
  if (on && !s->ev_copy) HIPCHK(hipEventCreateWithFlags(&s->ev_copy, hipEventDisableTiming));
  // bnd_mode 2: the pair kernels' boundary launch on its own stream beside their interior launch
  // (run_pair); a stage launch's boundary runs before its interior.  3 (round 5's default): the
  // boundary pipeline -- as 2, and the halo waits on the boundary stream (pft_slab_halo_wait), so
  // that no pair interior launch waits for a neighbour's flag (profiles/r05_ce_shapes.txt: +1% over 2
  // on one GPU).  5 (default since round 6): one pair launch per exchange, no boundary launch --
  // pair 2+3 with every tile column's first and last z-chunk leading the grid (PFT_K_ENDS_FIRST),
  // pair 4+5 with two-plane boundary chunks leading its interior chunks (PFT_K_INLINE, see
  // pft_slab_pair_inline); the copies start behind bnd_trigger_kernel once those workgroups are
  // done, while the rest of the launch runs.  The interior launch of 2 / 3 holds the CUs for
  // several rounds of workgroups on the driver's N > 1 slabs, so their boundary launch beside it
  // ran late and its copies after it (profiles/r06_ce_shapes.txt).  4: placement 4 for both pairs.
  // Stage launches keep their boundary first (inline with PFT_CE_STAGE_INLINE=1: slower, the
  // boundary workgroups' write-backs in a 3-workgroups-per-CU launch).  Env overrides for A/B
  // (profiles/r05_ce_ab.txt, r05_ce_shapes.txt, r06_ce_shapes.txt): PFT_CE_BND=2 the
  // waits on the compute stream, 0 every boundary before its interior, 1 every one beside (slower:
  // a stage launch's interior fills the chip, the two launches' workgroups are dealt interleaved
  // and the boundary ends late, profiles/r05_ce_trace_bnd.txt); PFT_CE_STREAMS=1 puts every copy
  // on the comm stream (slower)
  const char* eb = getenv("PFT_CE_BND");
  const char* es = getenv("PFT_CE_STREAMS");
  s->bnd_mode = !on ? 0 : eb && atoi(eb) >= 0 && atoi(eb) <= 5 ? atoi(eb) : 5;
  if (s->bnd_mode >= 4 && !s->bdone) {
    HIPCHK(hipMalloc((void**)&s->bdone, 64));
    HIPCHK(hipMemsetAsync(s->bdone, 0, 64, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->bdone_target = 0;
    HIPCHK(hipEventCreateWithFlags(&s->ev_trig, hipEventDisableTiming));
  }
  s->inline_pending = 0;
  {
    const char* et = getenv("PFT_CE_TRIG");
    const char* esi = getenv("PFT_CE_STAGE_INLINE");
    s->trig_early = et ? atoi(et) != 0 : 1;
    s->stage_inline = esi ? atoi(esi) != 0 : 0;
  }
  {
    // CUs reserved for the boundary launches (PFT_CE_RESERVE=R): the compute stream is re-created
    // with a CU mask that leaves R CUs out, so an interior launch of several rounds of workgroups
    // can never hold the CUs the boundary launch beside it needs.  R/8 per XCD, chosen so that
    // either numbering of the mask (CU-major per XCD or XCD-interleaved) spreads them evenly.
    const char* er = getenv("PFT_CE_RESERVE");
    const int want = on && s->bnd_mode >= 2 && er ? atoi(er) : 0;
    if (want != s->cu_reserved && want >= 0 && want <= 32 && want % 8 == 0 && s->n_cu == 256) {
      uint32_t mask[8];
      for (int w = 0; w < 8; ++w) mask[w] = ~0u;
      for (int x = 0; x < 8; ++x)
        for (int j = 0; j < want / 8; ++j) {
          const int bit = 32 * x + 8 * j + x;   // residue x mod 8, in the block of 32 numbered x
          mask[bit / 32] &= ~(1u << (bit % 32));
        }
      hipStream_t ns = nullptr;
      HIPCHK(hipStreamSynchronize(s->stream));
      HIPCHK(hipExtStreamCreateWithCUMask(&ns, 8, mask));
      HIPCHK(hipStreamDestroy(s->stream));
      s->stream = ns;
      s->cu_reserved = want;
    }
  }
  s->ce_streams = es && atoi(es) == 1 ? 1 : 2;
  if (s->ce_streams == 2 && !s->ev_copy) HIPCHK(hipEventCreateWithFlags(&s->ev_copy, hipEventDisableTiming));
  if (!s->ev_side) HIPCHK(hipEventCreateWithFlags(&s->ev_side, hipEventDisableTiming));
  if (!s->ev_join) HIPCHK(hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming));
  s->bnd_pending = 0;
  return 0;
}

int pft_slab_halo_signal(pft_slab* s, unsigned long long seq)
{
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_halo_signal");
  if (s->drop_puts) return 0;
  unsigned long long* slo = s->peer[0].on ? s->peer[0].sig + 1 : nullptr;   // below: its "from above"
  unsigned long long* shi = s->peer[1].on ? s->peer[1].sig + 0 : nullptr;   // above: its "from below"
  if (!slo && !shi) return 0;
  halo_signal_kernel<<<1, 64, 0, s->stream>>>(slo, shi, seq,
                                              s->peer[0].remote || s->peer[1].remote || s->peer[0].staged || s->peer[1].staged);
  HIPCHK(hipGetLastError());
  return 0;
}

int pft_slab_halo_wait(pft_slab* s, unsigned long long seq)
{
  // flags [0] (from below) and [1] (from above): the stream goes on once both planes are in
  if (s->ipc_poisoned) return slab_poisoned(s, "pft_slab_halo_wait");
  // the boundary pipeline (bnd_mode 3): after a boundary launch beside the interior, the flags are
  // waited for on the boundary stream -- only the next boundary launch (after this wait on that
  // stream) reads ghost planes; the next interior launch waits for this boundary launch alone
  hipStream_t ws = s->stream;
  if (s->bnd_pending) {
    // the boundary launch ran beside the interior one: its planes are the next launch's input
    HIPCHK(hipStreamWaitEvent(s->stream, s->ev_bnd, 0));
    s->bnd_pending = 0;
    if (s->bnd_mode == 3) ws = s->bnd;
  } else if (s->bnd_split && s->bnd_mode == 3 && s->bnd) {
    // a boundary launch before its interior (stage 1): its flags too are waited for on the
    // boundary stream, which the next boundary launch follows (run_pair beside, run_stage joins)
    ws = s->bnd;
  }
  s->bnd_split = 0;
  int sides = 0;
  WaitArgs w;
  memset(&w, 0, sizeof(w));
  w.seq = seq;
  for (int side = 0; side < 2; ++side) {
    if (!s->peer[side].on) continue;
    (side == 0 ? w.f0 : w.f1) = s->sig + side;
    if (s->peer[side].staged) sides |= 1 << side;
  }
  if (!w.f0 && !w.f1) return 0;
  int local_staged = 0;
  for (int side = 0; side < 2; ++side)
    if (((sides >> side) & 1) && !s->peer[side].remote) local_staged = 1;
  int blocks = 1;
  if (sides) {
    // staged: what the neighbours put into the receive buffer, into the ghost planes of the
    // exchange's buffer (the one the last halo_put2 sent: every rank runs the same sequence)
    RecvArgs& r = w.r;
    r.rbuf = s->rbuf + (long)(seq & 1) * 12 * s->plane;
    r.dst = s->buf[s->put_role];
    r.fs = s->fs;
    r.plane = s->plane;
    r.n3 = s->d.n3;
    r.f0 = s->put_f0;
    r.nf = s->put_f1 - s->put_f0;
    r.depth = s->put_deep ? 2 : 1;
    r.sides = sides;
    w.recv = 1;
    blocks = pft_halo_wait_blocks(4L * r.nf * s->plane, local_staged, s->gpu_ranks, ws == s->bnd);
  }
  if (s->wait_streamops) {
    // A/B (PFT_WAIT_STREAMOPS=1): the runtime's stream waits, then a separate receive launch
    for (int side = 0; side < 2; ++side)
      if (s->peer[side].on) HIPCHK(hipStreamWaitValue64(ws, s->sig + side, seq, hipStreamWaitValueGte, ~0ULL));
    if (sides) halo_recv_kernel<<<blocks, 256, 0, ws>>>(w.r);
  } else {
    halo_wait_kernel<<<blocks, 256, 0, ws>>>(w);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// Workgroups of one halo_wait_kernel launch with a staged receive of n doubles.  Every block spins
// on the flags before it copies, so the count bounds the CUs a wait can hold while the neighbour
// whose launch raises the flag may need them:
//  - a staged neighbour on this same GPU (PFT_IPC_STAGED between processes), or any other rank
//    sharing this GPU (gpu_ranks > 1: N ranks per GPU, whose neighbours may sit on another GPU and
//    depend on a rank of ours): 32 blocks.  A thousand spinning blocks would leave no CU for a pair
//    kernel's workgroup (the whole register file of a CU) of the rank that raises the flag, which
//    then waits out PFT_IPC_TIMEOUT -- or, across two GPUs, closes a wait cycle through both;
//  - in the boundary pipeline (the wait beside an interior launch that does not wait for it): 128
//    blocks of 4 waves, 16 CUs' worth; the 20 MB of the receive still take ~10 us;
//  - otherwise (this rank alone on its GPU, waiting on the compute stream): up to 1024.
int pft_halo_wait_blocks(long n, int local_staged, int gpu_ranks, int on_boundary_stream)
{
  int blocks = (int)std::min<long>(1024, std::max<long>(1, (n + 255) / 256));
  if (local_staged || gpu_ranks > 1) blocks = std::min(blocks, 32);
  if (on_boundary_stream) blocks = std::min(blocks, 128);
  return blocks;
}

int pft_slab_set_gpu_ranks(pft_slab* s, int n)
{
  if (!s || n < 1) return -2;
  s->gpu_ranks = n;
  return 0;
}

}  // extern "C"
