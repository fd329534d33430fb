"""Helpers of the f11 region tests (tests/test_region_host.py, tests/test_region_gpu.py): the
selections every shape is tried with, the region image restated in numpy, the host twin, grids of
any decomposition, and a bare pft_slab's region exports."""
import ctypes as C
import os

import numpy as np

import _snap as S
import porousfreezethaw_amd as P

ALL = slice(None)

# the k selections of the 3-slab tests on 7 planes (slabs of 3, 2, 2): one plane per rank; rank 0
# only; ranks 0 and 2 with none for rank 1; rank 1 only
K_SELECTIONS = [slice(1, 7, 2), slice(2, 3), slice(0, 7, 5), slice(4, 7, 3)]
K_OWNERS = [[1, 1, 1], [1, 0, 0], [1, 0, 1], [0, 1, 0]]


def _off(n, stride):
    """a start from which `stride` does not divide the remaining extent (0 when none exists)"""
    for start in range(min(stride, n)):
        if (n - start) % stride:
            return start
    return 0


def selections(n1, n2, n3):
    """[(name, (k, j, i))] on an n1 x n2 x n3 grid, numpy's way"""
    return [
        ("yz", (ALL, ALL, n1 // 2)),                                     # c1 == 1: rows of one word
        ("xz", (ALL, n2 // 2, ALL)),
        ("plane", (n3 // 2, ALL, ALL)),
        ("cell", (n3 - 1, 0, n1 // 3)),
        ("box_to_the_end", (slice(max(n3 - 2, 0), None), slice(n2 - 3, None), slice(n1 - 4, None))),
        ("stride2", (slice(_off(n3, 2), None, 2), slice(_off(n2, 2), None, 2), slice(_off(n1, 2), None, 2))),
        ("stride3", (slice(_off(n3, 3), None, 3), slice(_off(n2, 3), None, 3), slice(_off(n1, 3), None, 3))),
        ("stride_past_the_end", (slice(1, None, n3 + 5), slice(2, None, n2), slice(3, None, n1))),
        ("odd_i0", (ALL, slice(1, None), slice(1, None))),              # stride[0] == 1, rows start at odd words
        ("whole", (ALL, ALL, ALL)),                                      # the f7 dispatch
    ]


def as_index(sel):
    """the numpy index that keeps every axis: an int n (not negative here) becomes n:n+1"""
    return tuple(s if isinstance(s, slice) else slice(s, s + 1) for s in sel)


def grid(n1, n2, total_n3, nprocs=1, rank=0):
    """pft_grid of any slab of the driver's decomposition, filled in by hand (pft_grid_init refuses
    slabs of fewer than two planes, which the region arithmetic must still get right)"""
    g = P.pft_grid()
    n3, first = P.decompose(total_n3, nprocs, rank)
    g.n1, g.n2, g.n3, g.total_n3, g.first_row, g.rank, g.nprocs = n1, n2, n3, total_n3, first, rank, nprocs
    g.L1, g.L2, g.L3 = 0.03, 0.05, 0.07
    return g


def local(g, r):
    """(kfirst, kcount, klocal) of pft_region_local"""
    a, b, c = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    rc = P.lib().pft_region_local(C.byref(g), C.byref(r), C.byref(a), C.byref(b), C.byref(c))
    assert rc == 0, rc
    return a.value, b.value, c.value


def host_image(g, r, w):
    """pft_region_image_host of the padded array w (bytes)"""
    n = P.lib().pft_region_image_bytes(C.byref(g), C.byref(r))
    out = C.create_string_buffer(n + 8)
    assert P.lib().pft_region_image_host(C.byref(g), C.byref(r), P._dp(w), out) == 0
    assert out.raw[n:] == b"\0" * 8
    return out.raw[:n]


def be_words(b):
    return np.frombuffer(b, ">u8")


def ranges(path, g, r):
    out = P.pft_snapshot_ranges()
    rc = P.lib().pft_snapshot_region_ranges(os.fsencode(path), C.byref(g), C.byref(r), C.byref(out))
    assert rc == 0, rc
    return out


def local_region(g, r):
    """r with its k triple made slab-local: what the slab's entries take"""
    _, kcount, klocal = local(g, r)
    loc = P.pft_region()
    for a in range(3):
        loc.start[a], loc.count[a], loc.stride[a] = r.start[a], r.count[a], r.stride[a]
    loc.start[2], loc.count[2] = klocal, kcount
    return loc


class Slab(S.Slab):
    """_snap.Slab with the region exports"""

    def region_device(self, which, loc, offset=0):
        """the region image through device memory (offset: bytes into the allocation, a multiple of 8)"""
        L, dev = self.L, C.c_void_p()
        n = L.pft_slab_region_image_bytes(C.byref(loc))
        assert L.pft_dev_alloc(C.byref(dev), n + 64) == 0
        try:
            rc = L.pft_slab_export_region_be(self.s, which, C.byref(loc), C.c_void_p(dev.value + offset))
            assert rc == 0, (rc, L.pft_hip_last_error())
            out = np.zeros(n // 8)
            stream = L.pft_slab_stream(self.s)
            assert L.pft_flat_d2h(P._dp(out), C.c_void_p(dev.value + offset), n // 8, stream) == 0
            assert L.pft_stream_sync(stream) == 0
            return out.tobytes()
        finally:
            L.pft_dev_free(dev)

    def region_pinned(self, which, loc, link):
        """the region image through the slab's pinned buffer, by host link 0 (direct) or 1 (staged)"""
        img = C.c_void_p()
        rc = self.L.pft_slab_region_export(self.s, which, C.byref(loc), link, C.byref(img))
        assert rc == 0, (rc, self.L.pft_hip_last_error())
        return C.string_at(img.value, self.L.pft_slab_region_image_bytes(C.byref(loc)))
