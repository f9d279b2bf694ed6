"""CPU test of the SHA256 / MD5 digest entry points of include/ozec.h: digest lengths, and every argument error
reported as OZEC_EINVAL with its message before any device is touched -- the same calls are repeated in a child process
that sees no GPU at all.  The CRC entry points keep refusing types 4 and 5."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from ozone_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHA256, MD5 = 4, 5


def _err():
    return L.last_error()


def test_constants_and_digest_length():
    assert (L.OZEC_CHECKSUM_SHA256, L.OZEC_CHECKSUM_MD5) == (SHA256, MD5)
    lib = L.lib()
    assert [lib.ozec_digest_length(t) for t in (4, 5, 3, 1)] == [32, 16, 0, 0]
    assert [lib.ozec_digest_length(t) for t in (2, 0, 6, -1)] == [0, 0, 0, 0]


def _calls(lib, typ, data, n, bpc, out, cells=1):
    """the four digest calls with the same arguments; `data` / `out` are host addresses passed where a device address is
    expected too, which is fine for calls that must fail before they touch a device"""
    mism = np.zeros(4, np.int32)
    return {
        "ozec_digest_windows": lambda: lib.ozec_digest_windows(typ, data, n, bpc, out),
        "ozec_digest_windows_device": lambda: lib.ozec_digest_windows_device(typ, data, n, bpc, out, None),
        "ozec_digest_windows_batch": lambda: lib.ozec_digest_windows_batch(typ, data, n, cells, n, bpc, out, None),
        "ozec_digest_verify_batch": lambda: lib.ozec_digest_verify_batch(typ, data, n, cells, n, bpc, out,
                                                                         mism.ctypes.data, None),
    }


def check_argument_errors():
    """every row of the argument-error table; runs here and in the GPU-less child process below"""
    lib = L.lib()
    buf = np.arange(256, dtype=np.uint8)
    out = np.full(64 + 64, 0xA5, np.uint8)
    d, o = buf.ctypes.data, out.ctypes.data
    for typ in (0, 1, 2, 3, 6, -1):  # NONE, the CRC types and values outside ChecksumType
        for name, call in _calls(lib, typ, d, 256, 64, o).items():
            assert call() == L.OZEC_EINVAL, (name, typ)
            assert "ozec_checksum_windows" in _err() and str(typ) in _err(), (name, typ, _err())
    for typ in (SHA256, MD5):
        for name, call in _calls(lib, typ, d, 256, 0, o).items():
            assert call() == L.OZEC_EINVAL, (name, typ)
            assert _err() == "bytesPerChecksum must be positive", (name, _err())
        for name, call in list(_calls(lib, typ, None, 256, 64, o).items()) + list(_calls(lib, typ, d, 256, 64, None).items()):
            assert call() == L.OZEC_EINVAL, (name, typ)
            assert "null" in _err(), (name, _err())
        mism = np.zeros(4, np.int32)
        assert lib.ozec_digest_verify_batch(typ, d, 256, 1, 256, 64, o, None, None) == L.OZEC_EINVAL
        assert "null" in _err()
        # nothing to do: OK, nothing written, whatever the pointers
        assert lib.ozec_digest_windows(typ, d, 0, 64, o) == L.OZEC_OK
        assert lib.ozec_digest_windows(typ, None, 0, 64, None) == L.OZEC_OK
        assert lib.ozec_digest_windows_device(typ, d, 0, 64, o, None) == L.OZEC_OK
        assert lib.ozec_digest_windows_batch(typ, d, 256, 0, 256, 64, o, None) == L.OZEC_OK
        assert lib.ozec_digest_windows_batch(typ, d, 256, 3, 0, 64, o, None) == L.OZEC_OK
        assert lib.ozec_digest_verify_batch(typ, d, 256, 0, 256, 64, o, mism.ctypes.data, None) == L.OZEC_OK
        assert lib.ozec_digest_verify_batch(typ, d, 256, 3, 0, 64, o, mism.ctypes.data, None) == L.OZEC_OK
        assert (out == 0xA5).all() and (mism == 0).all()
    return True


def test_argument_errors():
    assert check_argument_errors()


def test_argument_errors_with_no_device_present():
    """the same table in a process from which every GPU is hidden: the errors cannot have come from a device"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from ozone_amd import _lib as L\n"
            "import test_digest_abi as t\n"
            "assert L.lib().ozec_device_count() == 0\n"
            "assert t.check_argument_errors()\n"
            "print('argument errors OK without a device')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK without a device" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("typ", [SHA256, MD5])
def test_crc_entry_points_still_refuse_digest_types(typ):
    lib = L.lib()
    buf = np.arange(64, dtype=np.uint8)
    out = np.zeros(4, np.uint32)
    assert lib.ozec_checksum_windows(typ, buf.ctypes.data, 64, 16, out.ctypes.data, 0) == L.OZEC_EINVAL
    assert "unsupported checksum type" in _err()
    idx = ctypes.c_int64(0)
    assert lib.ozec_checksum_verify(typ, buf.ctypes.data, 64, 16, out.ctypes.data, 4, 0,
                                    ctypes.byref(idx)) == L.OZEC_EINVAL
    state = ctypes.c_uint32(0xFFFFFFFF)
    assert lib.ozec_crc_update(typ, ctypes.byref(state), buf.ctypes.data, 64) == L.OZEC_EINVAL
    assert state.value == 0xFFFFFFFF
