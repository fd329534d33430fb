"""Helpers of the f7 snapshot tests (tests/test_snapshot_host.py, tests/test_snapshot_device_gpu.py):
the image of a slab restated in numpy, states of random 64-bit patterns, datasets written by the
host path, and a bare pft_slab with the export / import calls."""
import ctypes as C
import os

import numpy as np

import _diag as D
import porousfreezethaw_amd as P

NEG_ZERO = 0x8000000000000000
SPECIALS = [0x7ff8000000000000, 0x7ff0000000000001, 0xfff4dead0000beef, 0x7ff0000000000000, 0xfff0000000000000,
            NEG_ZERO, 0x0000000000000000, 0x0000000000000001, 0x800fffffffffffff, 0x3ff0000000000000]


def np_image(a):
    """the image of an interior state a[3][n3][n2][n1]: per field the words, big-endian"""
    return b"".join(np.ascontiguousarray(a[q]).view("<u8").astype(">u8").tobytes() for q in range(3))


def random_words(n1, n2, n3, seed, clean_gl=False):
    """a state of random 64-bit patterns (as float64): NaN payloads, -0.0, subnormals and +-Inf are
    planted in every field; clean_gl: the gl field holds neither -0.0 nor NaN"""
    r = np.random.default_rng(seed)
    w = r.integers(0, 1 << 64, size=(3, n3, n2, n1), dtype=np.uint64)
    flat = w.reshape(3, -1)
    n = flat.shape[1]
    for q in range(3):
        for i, v in enumerate(SPECIALS):
            flat[q, (7 * i + 3 * q + 1) % n] = v
    if clean_gl:
        g = flat[2]
        bad = (g == NEG_ZERO) | ((g & np.uint64(0x7fffffffffffffff)) > np.uint64(0x7ff0000000000000))
        g[bad] = np.uint64(0x3fe0000000000000)
    return w.view(np.float64)


def words(a):
    return np.ascontiguousarray(a).view(np.uint64)


def host_image(g, w):
    """pft_snapshot_image_host of the padded array w"""
    n = P.lib().pft_snapshot_image_bytes(C.byref(g))
    out = C.create_string_buffer(n)
    assert P.lib().pft_snapshot_image_host(C.byref(g), P._dp(w), out) == 0
    return out.raw


def ranges(path, g):
    r = P.pft_snapshot_ranges()
    rc = P.lib().pft_snapshot_slab_ranges(os.fsencode(path), C.byref(g), C.byref(r))
    assert rc == 0, rc
    return r


def file_image(path, g):
    """the bytes this slab owns in the dataset, u, p, gl in turn"""
    r = ranges(path, g)
    with open(path, "rb") as f:
        out = []
        for q in range(3):
            f.seek(r.off[q])
            out.append(f.read(r.bytes))
    return b"".join(out)


def write_host(path, g, params, info, w, version=0):
    """a dataset by the host path: pft_snapshot_create + pft_snapshot_write_slab"""
    L = P.lib()
    assert L.pft_snapshot_create(os.fsencode(path), C.byref(g), P._dp(params), C.byref(info), version) == 0
    assert L.pft_snapshot_write_slab(os.fsencode(path), C.byref(g), P._dp(w)) == 0


class SlabDesc(C.Structure):
    """include/pft_hip.h pft_slab_desc"""
    _fields_ = [("n1", C.c_int), ("n2", C.c_int), ("n3", C.c_int), ("has_below", C.c_int),
                ("has_above", C.c_int), ("calc_mode", C.c_int), ("gl_static", C.c_int),
                ("eps_mult", C.c_double * 3)]


class Slab:
    """a bare pft_slab (no model, no solver): export and import touch the buffers only"""

    def __init__(self, n1, n2, n3):
        L = P.lib()
        L.pft_slab_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(SlabDesc), C.c_void_p]
        L.pft_slab_upload_host.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.pft_slab_download_host.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.pft_slab_destroy.argtypes = [C.c_void_p]
        L.pft_dev_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.pft_dev_free.argtypes = [C.c_void_p]
        L.pft_flat_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.pft_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.pft_stream_sync.argtypes = [C.c_void_p]
        self.L, self.shape = L, (3, n3, n2, n1)
        d = SlabDesc(n1, n2, n3, 0, 0, 0, 0, (C.c_double * 3)(1.0, 1.0, 1.0))
        consts = (C.c_double * 64)(*([1.0] * 64))     # pft_consts: doubles only, unused here
        self.s = C.c_void_p()
        rc = L.pft_slab_create(C.byref(self.s), C.byref(d), consts)
        assert rc == 0, (rc, L.pft_hip_last_error())
        self.bytes = L.pft_slab_image_bytes(self.s)
        assert self.bytes == 24 * n1 * n2 * n3

    def upload(self, which, w):
        assert self.L.pft_slab_upload_host(self.s, which, P._dp(w)) == 0

    def download(self, which, poison=True):
        """the padded host array of buffer `which` (the host's ghost cells are kept)"""
        w = D.padded(np.zeros(self.shape), poison)
        assert self.L.pft_slab_download_host(self.s, which, P._dp(w)) == 0
        return w

    def interior(self, which):
        _, n3, n2, n1 = self.shape
        return np.ascontiguousarray(self.download(which)[:, 2:2 + n3, 2:2 + n2, 2:2 + n1])

    def export_device(self, which, offset=0):
        """the image through device memory (offset: bytes into the allocation, a multiple of 8)"""
        L, dev = self.L, C.c_void_p()
        assert L.pft_dev_alloc(C.byref(dev), self.bytes + 64) == 0
        try:
            rc = L.pft_slab_export_be(self.s, which, C.c_void_p(dev.value + offset))
            assert rc == 0, (rc, L.pft_hip_last_error())
            out = np.zeros(self.bytes // 8)
            stream = L.pft_slab_stream(self.s)
            assert L.pft_flat_d2h(P._dp(out), C.c_void_p(dev.value + offset), self.bytes // 8, stream) == 0
            assert L.pft_stream_sync(stream) == 0
            return out.tobytes()
        finally:
            L.pft_dev_free(dev)

    def export_pinned(self, which, link):
        """the image through the slab's pinned buffer, by host link 0 (direct) or 1 (staged)"""
        img = C.c_void_p()
        rc = self.L.pft_slab_snapshot_export(self.s, which, link, C.byref(img))
        assert rc == 0, (rc, self.L.pft_hip_last_error())
        return C.string_at(img.value, self.bytes)

    def import_image(self, image):
        """image (bytes) through the slab's pinned buffer into X and XN; returns gl_unclean"""
        host, dev, flag = C.c_void_p(), C.c_void_p(), C.c_int(-1)
        assert self.L.pft_slab_image(self.s, C.byref(host), C.byref(dev)) == 0
        C.memmove(host.value, image, self.bytes)
        rc = self.L.pft_slab_import_be(self.s, dev, C.byref(flag))
        assert rc == 0, (rc, self.L.pft_hip_last_error())
        return flag.value

    def close(self):
        self.L.pft_slab_destroy(self.s)
