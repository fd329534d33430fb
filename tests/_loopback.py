"""Several z-slabs on one GPU for the tests: the loopback transport (pft_comm_init_loopback), one
host thread per slab.  libpft's solver, model and option state are per host thread, so the body
configures its own Simulation; PFT_OPT_PAIR is set for the thread before it runs."""
import ctypes as C
import threading

import porousfreezethaw_amd as P


def run_slabs(nprocs, body, pair=None):
    """body(rank) on nprocs host threads, each with its rank's loopback communicator current and,
    if pair is not None, PFT_OPT_PAIR = pair; returns the bodies' results in rank order and raises
    the first exception of any of them"""
    L = P.lib()
    group = C.c_void_p()
    assert L.pft_comm_init_loopback(C.byref(group), nprocs) == 0
    out, errs = [None] * nprocs, []

    def worker(r):
        try:
            mine = C.c_void_p()
            assert L.pft_comm_loopback_rank(group, r, C.byref(mine)) == 0
            L.pft_comm_set_current(mine)
            if pair is not None:
                L.pft_solver_set_option(P.PFT_OPT_PAIR, pair)
            out[r] = body(r)
            L.pft_solver_set_option(P.PFT_OPT_PAIR, 1)
            L.pft_comm_set_current(None)
            L.pft_comm_destroy(mine)
        except BaseException as e:   # noqa: BLE001 -- surfaced below
            errs.append(e)

    ths = [threading.Thread(target=worker, args=(r,)) for r in range(nprocs)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=600)
    L.pft_comm_destroy(group)
    if errs:
        raise errs[0]
    return out
