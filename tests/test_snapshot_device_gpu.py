"""f7 on the GPU: the export / import kernels (pft_slab_export_be, pft_slab_import_be) against the
host twin and numpy, word for word; snapshot files from the resident state (Simulation.snapshot_device)
against download() + save_snapshot byte for byte, synchronous and in the background; restarts read
on the device (Simulation(icond_file=...)) against the reference's golden trajectory, on one slab,
on loopback slabs and in two ipc processes; and a series continued through the front end against the
uninterrupted one."""
import ctypes as C
import filecmp
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import _diag as D
import _multi as M
import _oracle as O
import _snap as S
import porousfreezethaw_amd as P
from porousfreezethaw_amd import frontend as FE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
X, XN = P.PFT_BUF_X, P.PFT_BUF_XN


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


# ---- 1. slab level ---------------------------------------------------------------------------

# 7x5x3: 105 elements, below one wave, an odd run (a lone last element; the second field of the
# image starts at an 8-byte boundary only); 64x8x2: exactly 1 024 elements; 33x31x9: odd, several
# workgroups; 50x50x4: 10 000, five workgroups
GRIDS = [(7, 5, 3), (64, 8, 2), (33, 31, 9), (50, 50, 4)]


@pytest.mark.parametrize("n1,n2,n3", GRIDS)
def test_slab_image_equals_host_twin_and_numpy(n1, n2, n3):
    """random 64-bit patterns (NaN payloads, -0.0, subnormals, +-Inf) compared as words, from X and
    from XN, ghost planes poisoned; through device memory (at a 16-byte and at an 8-byte boundary)
    and through the pinned buffer by both host links; export then import gives the same words in X
    and XN"""
    g = D.grid(n1, n2, n3)
    slab = S.Slab(n1, n2, n3)
    try:
        for which, other, seed in ((X, XN, 41), (XN, X, 42)):
            a, b = S.random_words(n1, n2, n3, seed), S.random_words(n1, n2, n3, seed + 10)
            w = D.padded(a)
            slab.upload(which, w)
            slab.upload(other, D.padded(b))
            want = S.np_image(a)
            assert S.host_image(g, w) == want
            for got in (slab.export_device(which), slab.export_device(which, offset=8),
                        slab.export_pinned(which, 0), slab.export_pinned(which, 1)):
                assert np.array_equal(np.frombuffer(got, ">u8"), np.frombuffer(want, ">u8"))
            assert slab.export_device(other) == S.np_image(b)
            # the inverse: the image of `which` into X and XN
            unclean = slab.import_image(want)
            assert unclean == 1                 # random_words plants -0.0 and NaNs in gl
            for buf in (X, XN):
                assert np.array_equal(S.words(slab.interior(buf)), S.words(a))
    finally:
        slab.close()


@pytest.mark.parametrize("n1,n2,n3", GRIDS)
def test_import_reports_unclean_gl_exactly(n1, n2, n3):
    """gl_unclean is 1 exactly when a -0.0 or a NaN is planted in gl -- at the first and at the last
    element -- and never for u or p"""
    slab = S.Slab(n1, n2, n3)
    try:
        base = S.random_words(n1, n2, n3, 51, clean_gl=True)
        assert slab.import_image(S.np_image(base)) == 0
        n = n1 * n2 * n3
        for cell in (0, n - 1):
            for bits in (S.NEG_ZERO, 0x7ff8000000000000, 0xfff0000000000001):
                a = base.copy()
                S.words(a).reshape(3, -1)[2, cell] = bits
                assert slab.import_image(S.np_image(a)) == 1
                assert np.array_equal(S.words(slab.interior(XN)), S.words(a))
            for bits in (0x0000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x8000000000000001):
                a = base.copy()
                S.words(a).reshape(3, -1)[2, cell] = bits
                assert slab.import_image(S.np_image(a)) == 0
        assert slab.import_image(S.np_image(base)) == 0       # the flag does not carry over
    finally:
        slab.close()


# ---- solver level ----------------------------------------------------------------------------

def _g20(mode=0, **kw):
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    kw.setdefault("tau", 1.0)
    if "icond_file" not in kw:
        kw.setdefault("initial", A[f"traj_m{mode}_ic"])
    return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), mode, Pm,
                        tau_min=info["tau_min"], delta=info["delta"], **kw)


def _info(sim, final, snapshot=1, total=4, comment="f7"):
    return P.snapshot_info(sim.t, sim.h, final, sim.system.delta, sim.grid.calc_mode, snapshot=snapshot,
                           total_snapshots=total, comment=comment)


def test_device_file_equals_host_file(tmp_path):
    """golden g20 after a solve to t = 36 s: the file from the resident state is byte for byte the
    one download() + save_snapshot write, as CDF-1 and with CDF-2 forced; before a state is resident
    the call refuses and creates nothing"""
    _, A = O.load_case("g20")
    sim = _g20()
    try:
        early = str(tmp_path / "early.ncd")
        inf = _info(sim, 360.0)
        assert sim.lib.pft_solver_snapshot_write(os.fsencode(early), P._dp(sim.params), C.byref(inf), 0) == -3
        with pytest.raises(RuntimeError, match="resident"):
            sim.snapshot_device(early, inf)
        assert not os.path.exists(early)
        sim.solve_ex(36.0, 0, P.PFT_SOLVE_KEEP_DEVICE)
        inf = _info(sim, 360.0)
        dev = [str(tmp_path / f"dev{i}.ncd") for i in range(4)]
        sim.snapshot_device(dev[0], inf)
        sim.snapshot_device(dev[1], inf, link="direct")
        sim.snapshot_device(dev[2], inf, link="staged")
        sim.snapshot_device(dev[3], inf, version=2)
        sim.download()
        host, host2 = str(tmp_path / "host.ncd"), str(tmp_path / "host2.ncd")
        P.save_snapshot(sim, host, inf)
        S.write_host(host2, sim.grid, sim.params, inf, sim.x, version=2)
        assert np.array_equal(sim.interior(), A["traj_m0_state0"])
    finally:
        sim.close()
    for f in dev[:3]:
        assert filecmp.cmp(f, host, shallow=False)
    assert filecmp.cmp(dev[3], host2, shallow=False)
    assert open(host, "rb").read(4) == b"CDF\x01" and open(dev[3], "rb").read(4) == b"CDF\x02"
    assert not filecmp.cmp(host, host2, shallow=False)


def test_async_snapshot_is_a_snapshot_not_a_view(tmp_path):
    """snapshot_device(wait=False) at t = 36 s, a solve to 360 s at once, then snapshot_wait(): the
    file is the one a twin run wrote synchronously at 36 s"""
    files = []
    for asynchronous in (False, True):
        sim = _g20()
        try:
            sim.solve_ex(36.0, 0, P.PFT_SOLVE_KEEP_DEVICE)
            path = str(tmp_path / ("async.ncd" if asynchronous else "sync.ncd"))
            sim.snapshot_device(path, _info(sim, 360.0), wait=not asynchronous)
            sim.solve_ex(360.0, 0, P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE)
            if asynchronous:
                sim.snapshot_wait()
            files.append(path)
            assert sim.t == 360.0
        finally:
            sim.close()
    assert filecmp.cmp(files[0], files[1], shallow=False)
    # a failed background write is reported by the wait
    sim = _g20()
    try:
        sim.solve_ex(36.0, 0, P.PFT_SOLVE_KEEP_DEVICE)
        path = str(tmp_path / "gone.ncd")
        L = sim.lib
        g, r = sim.grid, P.pft_snapshot_ranges()
        sim.snapshot_device(path, _info(sim, 360.0))
        assert L.pft_snapshot_slab_ranges(os.fsencode(path), C.byref(g), C.byref(r)) == 0
        img = C.create_string_buffer(r.bytes * 3)
        assert L.pft_snapshot_write_image_async(os.fsencode(str(tmp_path / "no" / "dir.ncd")), C.byref(r), img) == 0
        with pytest.raises(OSError, match="background"):
            sim.snapshot_wait()
        sim.snapshot_wait()
    finally:
        sim.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pair", [0, 2])
def test_restart_on_the_device_reaches_the_golden_rows(mode, pair, tmp_path):
    """files of the golden g20 states at t = 36 s and t = 360 s, read with Simulation(icond_file=):
    diagnostics() answers at once and equals numpy on the file's state; the solves 36 -> 360 and
    360 -> 720 reach the reference's rows bit for bit (t, h, the step counts from the restart on)
    and its fields -- with one launch per stage and with the pair kernels"""
    meta, A = O.load_case("g20")
    rows = meta[f"traj_m{mode}"]
    P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, pair)
    try:
        for i in (0, 1):
            state, t, h = A[f"traj_m{mode}_state{i}"], float.fromhex(rows[i][0]), float.fromhex(rows[i][1])
            T = meta["traj_times"][i + 1]
            path = str(tmp_path / f"image.{i}.ncd")
            w = _g20(mode, initial=state, init_solver=False)
            P.save_snapshot(w, path, P.snapshot_info(t, h, T, w.system.delta, mode, snapshot=i + 1, total_snapshots=4))
            w.close()
            sim = _g20(mode, icond_file=path, t0=t, tau=h, tile=2)
            try:
                assert sim.ic_where == "device"
                d = sim.diagnostics()
                D.assert_same(d, D.np_diag(state)[0], "diagnostics right after the read")
                assert np.array_equal(sim.interior(), state)          # the host array received a copy
                sim.solve(T)
                assert sim.stats().path == 1 and sim.stats().pairs == (1 if pair else 0)
                ref = rows[i + 1]
                assert (sim.t.hex(), sim.h.hex(), rows[i][2] + sim.system.steps, rows[i][3] + sim.system.steps_total) == \
                    (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(), ref[2], ref[3])
                assert np.array_equal(sim.interior(), A[f"traj_m{mode}_state{i + 1}"])
            finally:
                sim.close()
    finally:
        P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, 1)


def test_dimension_mismatch_is_refused(tmp_path):
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    path = str(tmp_path / "a.ncd")
    w = _g20(initial=A["traj_m0_state0"], init_solver=False)
    P.save_snapshot(w, path, P.snapshot_info(36.0, 0.7, 360.0, 1e-3, 0))
    w.close()
    with pytest.raises(OSError, match=r"\(-4\)"):
        P.Simulation(info["n1"], info["n2"], info["n3"] + 2, (info["L1"], info["L2"], info["L3"]), 0, Pm,
                     icond_file=path)


# ---- 5. decomposition ------------------------------------------------------------------------

def _small(state_file, nprocs=1, rank=0):
    Pm = O.params_from_meta(O.load_case("g20")[0])[0]
    return P.Simulation(7, 5, 7, (0.03, 0.03, 0.06), 0, Pm, nprocs=nprocs, rank=rank, icond_file=state_file)


def test_loopback_slabs_write_and_read_one_file(tmp_path):
    """a 7x5x7 grid on 3 loopback slabs (3, 2, 2 planes of 35 cells: odd runs, images that start at
    odd words): every slab reads its planes of a dataset and writes them into a new one, byte for
    byte the first; that file is then read on 1 and on 2 slabs"""
    a = D.random_state(7, 5, 7, 61)
    a[2] = np.abs(a[2])
    Pm = O.params_from_meta(O.load_case("g20")[0])[0]
    first, second = str(tmp_path / "first.ncd"), str(tmp_path / "second.ncd")
    inf = P.snapshot_info(36.0, 0.5, 72.0, 1e-3, 0, snapshot=3, total_snapshots=9, comment="slabs")
    g = D.grid(7, 5, 7)
    g.L1, g.L2, g.L3 = 0.03, 0.03, 0.06
    S.write_host(first, g, Pm, inf, D.padded(a, poison=False))

    def rewrite(sim):
        sim.snapshot_device(second, inf, wait=False)
        sim.snapshot_wait()
        return sim.grid.n3, sim.interior()

    out = M.loopback_run(3, lambda r: _small(first, 3, r), rewrite)
    assert [o[0] for o in out] == [3, 2, 2]
    assert np.array_equal(np.concatenate([o[1] for o in out], axis=1), a)
    assert filecmp.cmp(first, second, shallow=False)
    one = _small(second)
    try:
        assert np.array_equal(one.interior(), a)
        D.assert_same(one.diagnostics(), D.np_diag(a)[0])
    finally:
        one.close()
    out = M.loopback_run(2, lambda r: _small(second, 2, r), lambda sim: (sim.interior(), sim.diagnostics()))
    assert np.array_equal(np.concatenate([o[0] for o in out], axis=1), a)
    for _, d in out:
        D.assert_same(d, D.np_diag(a)[0])


def test_two_ipc_processes_write_and_read(tmp_path):
    """2 processes over the ipc transport (tests/_ipc_snap_worker.py) read the golden state at 36 s,
    each its own planes, solve to 360 s and write one file from their resident slabs: byte for byte
    the single slab's"""
    meta, A = O.load_case("g20")
    ref0, ref1 = meta["traj_m0"][0], meta["traj_m0"][1]
    t, h = float.fromhex(ref0[0]), float.fromhex(ref0[1])
    start = str(tmp_path / "start.ncd")
    w = _g20(initial=A["traj_m0_state0"], init_solver=False)
    P.save_snapshot(w, start, P.snapshot_info(t, h, 360.0, w.system.delta, 0, snapshot=1, total_snapshots=4))
    w.close()
    one = _g20(icond_file=start, t0=t, tau=h)
    try:
        one.solve_ex(360.0, 0, P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE)
        single = str(tmp_path / "single.ncd")
        one.snapshot_device(single, P.snapshot_info(one.t, one.h, 360.0, one.system.delta, 0, snapshot=2,
                                                    total_snapshots=4, comment="ipc"))
        one.download()
        assert np.array_equal(one.interior(), A["traj_m0_state1"])
        assert (one.t.hex(), one.h.hex()) == (float.fromhex(ref1[0]).hex(), float.fromhex(ref1[1]).hex())
    finally:
        one.close()
    spec = {"nranks": 2, "shm": f"/pft_snap_{os.getpid()}_{uuid.uuid4().hex[:12]}", "icond_file": start, "t0": t,
            "tau": h, "T": 360.0, "out": str(tmp_path / "two.ncd"), "res": str(tmp_path / "rank")}
    path = tmp_path / "spec.json"
    path.write_text(json.dumps(spec))
    env = dict(os.environ, PFT_IPC_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_ipc_snap_worker.py"), str(path), str(r)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=240)
            outs.append(out.decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed ({p.returncode}):\n{outs[r][-3000:]}"
    want, _ = D.np_diag(A["traj_m0_state0"])
    for r in range(2):
        res = json.load(open(f"{spec['res']}.{r}.json"))
        D.assert_same(res["diag"], want, "the global record right after the read")
        assert (float(res["t"]).hex(), float(res["h"]).hex()) == (float.fromhex(ref1[0]).hex(), float.fromhex(ref1[1]).hex())
    assert filecmp.cmp(spec["out"], single, shallow=False)


# ---- 6. continuation through the front end ---------------------------------------------------

def test_continued_series_equals_the_uninterrupted_one(tmp_path):
    """the Params text of test_frontend_gpu.py with final_time 72 and saved_files 9 (every snapshot
    time exact in both formulas), files from the resident state, written in the background.  A
    second case adds `set icond_file = <image.003.ncd>` and `set continue_series`: its rows for
    snapshots 3-8 equal the first run's in t, h and the diagnostics, its files 003-008 are byte for
    byte the first run's, attributes included.

    The step counters: a dataset records no step counts (the reference's does not either), and
    system.steps / steps_total count from the start of a run, so the continued run's counters are
    the first run's minus their values at snapshot 3; that difference is what is compared."""
    from test_frontend_gpu import PARAMS
    text = PARAMS.replace("final_time      10*hours", "final_time      72").replace("saved_files     100",
                                                                                     "saved_files     9")
    assert text != PARAMS and "final_time      72" in text and "saved_files     9" in text
    d1, d2 = tmp_path / "full", tmp_path / "cont"
    d1.mkdir()
    d2.mkdir()
    case = FE.load_params(text=text, env={"OUTPUT": str(d1)})
    rows1 = case.run(beads=O.beads(), snapshot_path=case.settings["out_file"], comment=case.settings["comment"],
                     snapshot_where="device", snapshot_async=True)
    assert [r["snapshot"] for r in rows1] == list(range(9)) and rows1[-1]["t"] == 72.0
    assert [r["t"] for r in rows1] == [9.0 * s for s in range(9)]
    tail = f"set icond_file = {d1}/image.003.ncd\nset continue_series\n"
    case2 = FE.load_params(text=text.replace("n3 L3 * multiplier", "n3 0") + tail, env={"OUTPUT": str(d2)})
    assert case2.icond_mode == 1 and case2.continue_series and case2.n[2] == 0
    assert case2.series_start()[:4] == (3, 9, 27.0, 72.0)
    rows2 = case2.run(beads=O.beads(), snapshot_path=case2.settings["out_file"], comment=case2.settings["comment"],
                      snapshot_where="device", snapshot_async=True)
    assert [r["snapshot"] for r in rows2] == list(range(3, 9))
    for a, b in zip(rows2, rows1[3:]):
        assert (a["t"].hex(), a["h"].hex()) == (b["t"].hex(), b["h"].hex())
        assert (a["steps"], a["steps_total"]) == (b["steps"] - rows1[3]["steps"], b["steps_total"] - rows1[3]["steps_total"])
        D.assert_same({k: a[k] for k in D.FIELDS}, {k: b[k] for k in D.FIELDS}, f"snapshot {a['snapshot']}")
    assert rows2[-1]["steps"] > 0
    for s in range(9):
        assert os.path.exists(d1 / ("image.%03d.ncd" % s))
        assert os.path.exists(d2 / ("image.%03d.ncd" % s)) == (s >= 3)
    for s in range(3, 9):
        assert filecmp.cmp(d1 / ("image.%03d.ncd" % s), d2 / ("image.%03d.ncd" % s), shallow=False), s
