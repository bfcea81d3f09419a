"""CPU: the C ABI of the device-side build of the cell-ordered cloud (read_splat_cells_build): exported, scratch size query,
argument checks that fail before any device work.  Its results are checked on the GPU (tests/test_gpu_cells_build.py)."""
import ctypes as C

from read_amd import _lib

FAKE = 1 << 20          # a 256-byte aligned non-null address: the calls below fail on their arguments and never touch it


def test_symbols_are_exported():
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "read_splat_cells_build") and hasattr(L, "read_splat_cells_build_scratch_bytes")
    assert "read_splat_cells_build" in _lib.SIGNATURES and "read_splat_cells_build_scratch_bytes" in _lib.SIGNATURES


def test_scratch_bytes():
    L = _lib.lib()
    assert L.read_splat_cells_build_scratch_bytes(0) == 0
    assert L.read_splat_cells_build_scratch_bytes(-1) == 0
    assert L.read_splat_cells_build_scratch_bytes(1 << 32) == 0
    prev = 0
    for n in (1, 2, 1023, 1024, 1025, 4096, 4097, 5000, (1 << 20) - 1, (1 << 20) + 3, 30_000_000, 0xFFFFFFFE):
        s = L.read_splat_cells_build_scratch_bytes(n)
        assert s > 0 and s >= prev, (n, s, prev)
        assert s >= 8 * n                                           # one array of 64-bit keys
        assert s <= 8.5 * n + (1 << 16), (n, s)                     # about 8 bytes per point plus a small fixed part
        prev = s


def test_bad_arguments_fail_before_device_work():
    L = _lib.lib()
    n = 5000
    nbytes, sbytes = L.read_splat_cells_bytes(n), L.read_splat_cells_build_scratch_bytes(n)

    def call(xyz, blob, blob_bytes, scratch, scratch_bytes, count=n):
        rc = L.read_splat_cells_build(xyz, count, blob, blob_bytes, scratch, scratch_bytes, None)
        return rc, L.read_last_error().decode()

    for args in ((None, FAKE, nbytes, FAKE, sbytes), (FAKE, None, nbytes, FAKE, sbytes), (FAKE, FAKE, nbytes, None, sbytes)):
        rc, msg = call(*args)
        assert rc == -22 and "read_splat_cells_build" in msg and "null" in msg, (args, msg)
    rc, msg = call(FAKE, FAKE, nbytes - 1, FAKE, sbytes)                            # short blob
    assert rc == -22 and "read_splat_cells_build" in msg and str(nbytes) in msg, msg
    rc, msg = call(FAKE, FAKE, nbytes, FAKE, sbytes - 1)                            # short scratch
    assert rc == -22 and "read_splat_cells_build" in msg and "scratch" in msg and str(sbytes) in msg, msg
    for bad_n in (0, -5, 1 << 32):
        rc, msg = call(FAKE, FAKE, 1 << 40, FAKE, 1 << 40, count=bad_n)
        assert rc == -22 and "read_splat_cells_build" in msg and "out of range" in msg, (bad_n, msg)
    rc, msg = call(FAKE, FAKE + 16, nbytes, FAKE, sbytes)                           # blob not 256-byte aligned
    assert rc == -22 and "read_splat_cells_build" in msg and "aligned" in msg, msg
