"""f11 on the CPU: a slab's share of a region (pft_region_local) against a brute force over every
small decomposition; the host twin of the device's region image (pft_region_image_host) against
numpy, word for word; region datasets written by the host path and read with the independent
classic-format reader of tests/test_io.py; the refusals of P.region and of a restart from a region
dataset; and three virtual ranks writing one region file."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import _diag as D
import _oracle as O
import _region as R
import _snap as S
import porousfreezethaw_amd as P

SHAPES = [(7, 5, 7), (8, 6, 5), (33, 31, 9)]


def _params():
    meta, _ = O.load_case("g20")
    return O.params_from_meta(meta)[0]


def _info(snapshot=3):
    return P.snapshot_info(36.0, 0.5, 72.0, 1e-3, 0, snapshot=snapshot, total_snapshots=9, comment="f11")


def _netcdf():
    return pytest.importorskip("scipy.io").netcdf_file


# ---- pft_region_local ------------------------------------------------------------------------

def test_region_local_equals_the_brute_force():
    """every total_n3 <= 9 on 1-4 ranks (slabs of one plane and of none included) and every valid
    (start, count, stride): first index, count and slab-local plane equal the owner list's; the
    shares are disjoint, ordered, and sum to count[2]"""
    checked = 0
    for total in range(1, 10):
        for nprocs in range(1, 5):
            grids = [R.grid(3, 2, total, nprocs, r) for r in range(nprocs)]
            assert sum(g.n3 for g in grids) == total
            for start in range(total):
                for stride in range(1, total + 2):
                    for count in range(1, (total - 1 - start) // stride + 2):
                        r = P.pft_region((0, 0, start), (1, 1, count), (1, 1, stride))
                        assert P.lib().pft_region_check(C.byref(grids[0]), C.byref(r)) == 0
                        sel = [start + m * stride for m in range(count)]
                        nxt = 0
                        for g in grids:
                            mine = [m for m, k in enumerate(sel) if g.first_row <= k < g.first_row + g.n3]
                            kfirst, kcount, klocal = R.local(g, r)
                            assert kcount == len(mine), (total, nprocs, g.rank, start, count, stride)
                            assert kfirst == nxt, (total, nprocs, g.rank, start, count, stride)
                            if mine:
                                assert kfirst == mine[0] and klocal == sel[mine[0]] - g.first_row
                                assert mine == list(range(mine[0], mine[0] + kcount))
                            nxt = kfirst + kcount
                            checked += 1
                        assert nxt == count
    assert checked > 5000


def test_region_check_refuses_what_leaves_the_grid():
    g = R.grid(7, 5, 7)
    chk = lambda *a: P.lib().pft_region_check(C.byref(g), C.byref(P.pft_region(*a)))  # noqa: E731
    assert chk((1, 0, 2), (3, 5, 2), (2, 1, 3)) == 0
    assert chk((1, 0, 2), (4, 5, 2), (2, 1, 3)) == -2 and chk((1, 0, 2), (3, 6, 2), (2, 1, 3)) == -2
    assert chk((1, 0, 2), (3, 5, 3), (2, 1, 3)) == -2
    for a in range(3):
        for field, bad in ((0, -1), (1, 0), (2, 0), (2, -1)):
            t = [[1, 0, 2], [3, 5, 2], [2, 1, 3]]
            t[field][a] = bad
            assert chk(*map(tuple, t)) == -2, (a, field, bad)
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    bad = P.pft_region((0, 0, 0), (1, 1, 8), (1, 1, 1))
    assert P.lib().pft_region_local(C.byref(g), C.byref(bad), C.byref(a), C.byref(b), C.byref(c)) == -2
    assert P.lib().pft_region_image_bytes(C.byref(g), C.byref(bad)) == 0


# ---- P.region --------------------------------------------------------------------------------

def test_python_region_normalises_as_numpy_does():
    dims = (9, 31, 33)
    a = np.arange(9 * 31 * 33).reshape(dims)
    for name, sel in R.selections(33, 31, 9) + [("negative", (-1, slice(-4, None), slice(None, -2, 3))),
                                                ("clamped", (slice(2, 100), slice(-100, 3), slice(5, 6)))]:
        r = P.region(*sel, dims)
        want = a[R.as_index(tuple(s if isinstance(s, slice) else s % n for s, n in zip(sel, dims)))]
        assert (r.count[2], r.count[1], r.count[0]) == want.shape, name
        assert np.array_equal(a[r.selection()], want), name
        assert P.lib().pft_region_check(C.byref(R.grid(33, 31, 9)), C.byref(r)) == 0
    g = R.grid(33, 31, 9)
    assert bytes(P.region(1, 2, 3, g)) == bytes(P.region(1, 2, 3, dims))


@pytest.mark.parametrize("sel,what", [
    ((slice(0, 7, 0), slice(None), slice(None)), "zero"),
    ((slice(None), slice(None, None, -1), slice(None)), "positive"),
    ((slice(None), slice(None), slice(6, 2, -2)), "positive"),
    ((slice(3, 3), slice(None), slice(None)), "empty"),
    ((slice(None), slice(5, 9), slice(None)), "empty"),
    ((slice(None), slice(None), slice(4, 2)), "empty"),
    ((7, 0, 0), "past"), ((0, 5, 0), "past"), ((0, 0, 7), "past"), ((-8, 0, 0), "past"),
    ((0.5, 0, 0), "slice or an int"),
])
def test_python_region_refusals(sel, what):
    """a step of 0 or below, an empty slice, an index past the grid: ValueError, no device involved"""
    with pytest.raises(ValueError, match=what):
        P.region(*sel, (7, 5, 7))
    sim = P.Simulation(7, 5, 7, D.L3, 0, _params(), init_solver=False)
    try:
        for call in (lambda: sim.region(sel), lambda: sim.region(sel, where="host"),
                     lambda: sim.snapshot_device("never.ncd", _info(), region=sel),
                     lambda: P.save_snapshot(sim, "never.ncd", _info(), region=sel),
                     lambda: sim.run_series(1.0, 2, snapshot_path="never", regions={"a": sel})):
            with pytest.raises(ValueError, match=what):
                call()
        with pytest.raises(ValueError, match="three items"):
            sim.region((slice(None), 0))
    finally:
        sim.close()
    assert not os.path.exists("never.ncd")


# ---- the image -------------------------------------------------------------------------------

@pytest.mark.parametrize("n1,n2,n3", SHAPES)
def test_host_region_image_equals_numpy(n1, n2, n3):
    """random 64-bit patterns, every ghost cell poisoned: per field interior()[sel] as big-endian
    words, on one slab and on every slab of a decomposition"""
    a = S.random_words(n1, n2, n3, 71)
    for nprocs in (1, 2, 3):
        if n3 // nprocs < 2:
            continue
        for rank in range(nprocs):
            g = D.grid(n1, n2, n3, nprocs, rank)
            mine = a[:, g.first_row:g.first_row + g.n3]
            w = D.padded(mine)
            for name, sel in R.selections(n1, n2, n3):
                r = P.region(*sel, g)
                kfirst, kcount, _ = R.local(g, r)
                want = a[(slice(None),) + R.as_index(sel)][:, kfirst:kfirst + kcount]
                got = R.host_image(g, r, w)
                assert len(got) == 8 * want.size, (name, nprocs, rank)
                assert np.array_equal(R.be_words(got), R.be_words(S.np_image(want))), (name, nprocs, rank)


# ---- the dataset -----------------------------------------------------------------------------

@pytest.mark.parametrize("version", [0, 2])
def test_region_dataset_under_an_independent_reader(version, tmp_path):
    """dimensions, coordinate variables bit-equal to the full dataset's at the selected indices, the
    attributes in a full dataset's order with the three region attributes last, the variables equal
    to interior()[sel]; pft_snapshot_read_info reads it"""
    from test_io import ATTR_ORDER
    netcdf = _netcdf()
    n1, n2, n3 = 33, 31, 9
    a = D.random_state(n1, n2, n3, 72)
    sim = P.Simulation(n1, n2, n3, (0.03, 0.05, 0.07), 0, _params(), initial=a, init_solver=False)
    try:
        full = str(tmp_path / "full.ncd")
        P.save_snapshot(sim, full, _info())
        with netcdf(full, "r", mmap=False) as f:
            coords = {v: f.variables[v][:].copy() for v in ("n3", "n2", "n1")}
            full_attrs = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in f._attributes.items()}
        for name, sel in R.selections(n1, n2, n3):
            path = str(tmp_path / f"{name}.ncd")
            P.save_snapshot(sim, path, _info(), region=sel, version=version)
            idx = R.as_index(sel)
            r = P.region(*sel, sim.grid)
            with netcdf(path, "r", mmap=False) as f:
                assert f.version_byte == (2 if version == 2 else 1)
                want = a[(slice(None),) + idx]
                assert list(f.dimensions.items()) == [("n3", want.shape[1]), ("n2", want.shape[2]), ("n1", want.shape[3])]
                assert list(f.variables) == ["n3", "n2", "n1", "u", "p", "gl"]
                assert list(f._attributes) == ATTR_ORDER + ["region_start", "region_count", "region_stride"]
                for axis, v in enumerate(("n3", "n2", "n1")):
                    got = np.ascontiguousarray(f.variables[v][:])
                    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(coords[v][idx[axis]]).view(np.uint64)), (name, v)
                for q, v in enumerate(("u", "p", "gl")):
                    assert np.array_equal(S.words(f.variables[v][:].astype("<f8")), S.words(want[q])), (name, v)
                at = f._attributes
                assert list(at["region_start"]) == list(r.start) and list(at["region_count"]) == list(r.count)
                assert list(at["region_stride"]) == list(r.stride)
                assert at["region_start"].dtype == np.dtype(">i4")
                for k in ATTR_ORDER:
                    assert np.array_equal(at[k], full_attrs[k]), k
            d1, d2, d3, info, prm = P.read_snapshot_info(path)
            assert (d3, d2, d1) == want.shape[1:]
            assert (info.t, info.tau, info.snapshot, info.total_snapshots) == (36.0, 0.5, 3, 9)
            assert info.title == _info().title and np.array_equal(prm, sim.params)
            assert P.read_snapshot_series(path) == (0, 3, 9, 36.0, 72.0, 0.5)
    finally:
        sim.close()


def test_full_dataset_is_unchanged_and_bad_arguments(tmp_path):
    """a full dataset carries no region attribute; create_region refuses a bad region and creates
    nothing; ranges against a dataset of other dimensions are -4"""
    g = D.grid(7, 5, 7)
    w = D.padded(D.random_state(7, 5, 7, 73))
    full, reg = str(tmp_path / "full.ncd"), str(tmp_path / "reg.ncd")
    S.write_host(full, g, _params(), _info(), w)
    assert b"region_" not in open(full, "rb").read()
    L = P.lib()
    bad = P.pft_region((0, 0, 0), (8, 5, 7), (1, 1, 1))
    inf = _info()
    assert L.pft_snapshot_create_region(os.fsencode(reg), C.byref(g), C.byref(bad), P._dp(_params()), C.byref(inf), 0) == -2
    assert not os.path.exists(reg)
    r = P.region(slice(1, 7, 2), 2, slice(None), g)
    assert L.pft_snapshot_create_region(os.fsencode(reg), C.byref(g), C.byref(r), P._dp(_params()), C.byref(inf), 0) == 0
    out = P.pft_snapshot_ranges()
    other = P.region(slice(1, 7, 3), 2, slice(None), g)
    assert L.pft_snapshot_region_ranges(os.fsencode(reg), C.byref(g), C.byref(other), C.byref(out)) == -4
    assert L.pft_snapshot_region_ranges(os.fsencode(full), C.byref(g), C.byref(r), C.byref(out)) == -4
    assert L.pft_snapshot_region_ranges(os.fsencode(reg), C.byref(g), C.byref(bad), C.byref(out)) == -2
    assert L.pft_snapshot_region_ranges(os.fsencode(reg), C.byref(g), C.byref(r), C.byref(out)) == 0
    assert out.bytes == 8 * 3 * 1 * 7
    # ranges of no bytes: nothing is opened, nothing written, also in the background
    none = P.pft_snapshot_ranges((0, 0, 0), 0)
    gone = os.fsencode(str(tmp_path / "no" / "dir.ncd"))
    assert L.pft_snapshot_write_image(gone, C.byref(none), None) == 0
    assert L.pft_snapshot_read_image(gone, C.byref(none), None) == 0
    assert L.pft_snapshot_write_image_async(gone, C.byref(none), None) == 0
    assert L.pft_snapshot_writer_wait() == 0
    assert L.pft_snapshot_write_image(os.fsencode(reg), C.byref(out), None) == -2


def test_restart_from_a_region_dataset_is_refused(tmp_path):
    """its dimensions differ from the grid's: -4 from the ranges, from the host reader, and from
    Simulation(icond_file=) before any solver work; the whole grid at stride 1 is still a region
    dataset (it carries the attributes) and restarts as any dataset does"""
    a = D.random_state(7, 5, 7, 74)
    sim = P.Simulation(7, 5, 7, D.L3, 0, _params(), initial=a, init_solver=False)
    try:
        part, whole = str(tmp_path / "part.ncd"), str(tmp_path / "whole.ncd")
        P.save_snapshot(sim, part, _info(), region=(slice(None), 2, slice(None)))
        P.save_snapshot(sim, whole, _info(), region=(slice(None), slice(None), slice(None)))
        out = P.pft_snapshot_ranges()
        assert P.lib().pft_snapshot_slab_ranges(os.fsencode(part), C.byref(sim.grid), C.byref(out)) == -4
        with pytest.raises(OSError, match=r"\(-4\)"):
            P.load_snapshot(sim, part)
        with pytest.raises(OSError, match=r"\(-4\)"):
            P.Simulation(7, 5, 7, D.L3, 0, _params(), icond_file=part)
        assert b"region_stride" in open(whole, "rb").read()
        assert P.lib().pft_snapshot_slab_ranges(os.fsencode(whole), C.byref(sim.grid), C.byref(out)) == 0
        sim.set_interior(np.zeros_like(a))
        P.load_snapshot(sim, whole)
        assert np.array_equal(sim.interior(), a)
    finally:
        sim.close()


# ---- three virtual ranks ---------------------------------------------------------------------

@pytest.mark.parametrize("ksel,owners", list(zip(R.K_SELECTIONS, R.K_OWNERS)))
def test_three_virtual_ranks_write_the_single_ranks_file(ksel, owners, tmp_path):
    """7x5x7 on slabs of 3, 2 and 2 planes: each rank's region_ranges + write_image of its host image
    -- a rank without a share writes nothing -- give the file the single rank writes"""
    a = S.random_words(7, 5, 7, 75)
    one = D.grid(7, 5, 7)
    L = P.lib()
    sel = (ksel, slice(1, None, 2), slice(0, None, 3))
    r = P.region(*sel, one)
    single, shared = str(tmp_path / "single.ncd"), str(tmp_path / "shared.ncd")
    inf = _info()
    rc = L.pft_snapshot_write_region(os.fsencode(single), C.byref(one), C.byref(r), P._dp(_params()), C.byref(inf),
                                     P._dp(D.padded(a)), 0)
    assert rc == 0
    assert L.pft_snapshot_create_region(os.fsencode(shared), C.byref(one), C.byref(r), P._dp(_params()), C.byref(inf), 0) == 0
    assert not filecmp.cmp(single, shared, shallow=False)
    counts = []
    for rank in (2, 0, 1):
        g = D.grid(7, 5, 7, 3, rank)
        assert g.n3 == (3, 2, 2)[rank]
        rg = R.ranges(shared, g, r)
        kfirst, kcount, _ = R.local(g, r)
        counts.append((rank, kcount))
        img = R.host_image(g, r, D.padded(a[:, g.first_row:g.first_row + g.n3]))
        assert len(img) == 3 * rg.bytes == 24 * kcount * r.count[1] * r.count[0]
        assert L.pft_snapshot_write_image(os.fsencode(shared), C.byref(rg), img if img else None) == 0
    assert [c for _, c in sorted(counts)] == owners
    assert filecmp.cmp(single, shared, shallow=False)
    whole = R.ranges(single, one, r)
    back = C.create_string_buffer(3 * whole.bytes)
    assert L.pft_snapshot_read_image(os.fsencode(single), C.byref(whole), back) == 0
    want = a[(slice(None),) + R.as_index(sel)]
    assert np.array_equal(R.be_words(back.raw), R.be_words(S.np_image(want)))
