"""CPU test of the stripe entry points that take ChecksumType SHA256 / MD5 (include/ozec.h: ozec_encode_digest_batch,
ozec_reconstruct_digest_batch, their _host_batch forms, ozec_stripe_queue_submit_digests and ozec_stripe_queue_create).

Argument errors come back before any device is touched, so the table runs here and again in a child process that sees no
GPU.  A coder or a queue cannot exist without a device (ozec_encoder_create answers OZEC_EDEVICE), so the rows that
need one -- closed coder, encoder where a decoder is wanted, null buffers, the two queue cross-errors -- are in
tests/test_gpu_stripe_digest.py; what needs none is here: the checksum type (a CRC or NONE type names the _crc_
counterpart), bytesPerChecksum == 0, a null coder, a null queue, and that nothing is written.  The Python
StripeQueue.submit(digests=...) buffer checks run before the library is called and are tested on a queue object that
never reaches it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ozone_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHA256, MD5 = 4, 5


def _calls(lib, coder, typ, bpc, bufs):
    """every new coder-taking export with the same arguments (host addresses stand in for device addresses: the calls
    must fail before they touch either); -> {name: (call, name of the CRC counterpart)}"""
    d, o, g, e, m, ints = bufs
    S, n = 2, 64
    return {
        "ozec_encode_digest_batch": (
            lambda: lib.ozec_encode_digest_batch(coder, d, 5 * n, n, o, 2 * n, n, S, n, typ, bpc, g, None),
            "ozec_encode_crc_batch"),
        "ozec_encode_digest_host_batch": (
            lambda: lib.ozec_encode_digest_host_batch(coder, d, 5 * n, n, o, 2 * n, n, S, n, typ, bpc, g, 0),
            "ozec_encode_crc_host_batch"),
        "ozec_reconstruct_digest_batch": (
            lambda: lib.ozec_reconstruct_digest_batch(coder, d, 5 * n, n, ints, 3, ints, 1, o, n, n, S, n, typ, bpc, e, g,
                                                      m, None),
            "ozec_reconstruct_crc_batch"),
        "ozec_reconstruct_digest_host_batch": (
            lambda: lib.ozec_reconstruct_digest_host_batch(coder, d, 5 * n, n, ints, 3, ints, 1, o, n, n, S, n, typ, bpc,
                                                           e, g, m, 0),
            "ozec_reconstruct_crc_host_batch"),
    }


def check_argument_errors():
    """every row that needs no coder; runs here and in the GPU-less child process below"""
    import ctypes
    lib = L.lib()
    data = np.arange(1024, dtype=np.uint8)
    out = np.full(1024, 0xA5, np.uint8)
    dig = np.full(4096, 0xA5, np.uint8)
    exp = np.full(4096, 0xA5, np.uint8)
    mis = np.full(8, 0x5A5A5A5A, np.int32)
    ints = (ctypes.c_int * 4)(1, 2, 3, 0)
    bufs = (data.ctypes.data, out.ctypes.data, dig.ctypes.data, exp.ctypes.data, mis.ctypes.data, ints)
    for typ in (0, 1, 2, 3, 6, -1):  # NONE, the CRC types and values outside ChecksumType: the message names the twin
        for name, (call, twin) in _calls(lib, None, typ, 16, bufs).items():
            assert call() == L.OZEC_EINVAL, (name, typ)
            assert twin in L.last_error() and str(typ) in L.last_error(), (name, typ, L.last_error())
    for typ in (SHA256, MD5):
        for name, (call, _) in _calls(lib, None, typ, 0, bufs).items():
            assert call() == L.OZEC_EINVAL, (name, typ)
            assert L.last_error() == "bytesPerChecksum must be positive", (name, L.last_error())
        for name, (call, _) in _calls(lib, None, typ, 16, bufs).items():
            assert call() == L.OZEC_EINVAL, (name, typ)
            assert L.last_error() == "null coder", (name, L.last_error())
    # the queue: no queue, no encoder
    ptrs = L.ptr_array([data.ctypes.data] * 3)
    t = ctypes.c_uint64(7)
    assert lib.ozec_stripe_queue_submit_digests(None, ptrs, ptrs, 64, dig.ctypes.data, ctypes.byref(t)) == L.OZEC_EINVAL
    assert L.last_error() == "null queue"
    q = ctypes.c_void_p(0x1234)
    for typ in (SHA256, MD5):
        assert lib.ozec_stripe_queue_create(None, 64, 4, typ, 16, 0, ctypes.byref(q)) != L.OZEC_OK
        assert not q.value
    assert t.value == 7
    assert (out == 0xA5).all() and (dig == 0xA5).all() and (exp == 0xA5).all() and (mis == 0x5A5A5A5A).all()
    return True


def test_argument_errors():
    assert check_argument_errors()


def test_argument_errors_with_no_device_present():
    """the same table in a process from which every GPU is hidden: the errors cannot have come from a device"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from ozone_amd import _lib as L\n"
            "import test_stripe_digest_abi as t\n"
            "assert L.lib().ozec_device_count() == 0\n"
            "assert t.check_argument_errors()\n"
            "print('argument errors OK without a device')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK without a device" in r.stdout, r.stdout + r.stderr


def test_new_exports_are_declared_and_bound():
    names = ["ozec_encode_digest_batch", "ozec_reconstruct_digest_batch", "ozec_encode_digest_host_batch",
             "ozec_reconstruct_digest_host_batch", "ozec_stripe_queue_submit_digests"]
    syms = L.header_symbols()
    for n in names:
        assert n in syms and n in L._SIGS and getattr(L.lib(), n) is not None, n


class _Enc:
    class _config:
        @staticmethod
        def get_codec():
            return "rs"

    @staticmethod
    def get_num_data_units():
        return 3

    @staticmethod
    def get_num_parity_units():
        return 2


def _queue_without_library(typ, bpc):
    """a StripeQueue as its constructor leaves it, without the native queue (which needs a device): submit() checks its
    buffers before it calls the library"""
    from ozone_amd.stripe_queue import StripeQueue
    q = StripeQueue.__new__(StripeQueue)
    q._enc, q._k, q._p, q._units, q._bpc = _Enc, 3, 2, 5, bpc
    q._dl = int(L.lib().ozec_digest_length(typ))
    q._h = None
    return q


@pytest.mark.parametrize("typ,dl", [(SHA256, 32), (MD5, 16)])
def test_python_submit_rejects_bad_digest_buffers(typ, dl):
    from ozone_amd.rawcoder import IllegalArgumentException
    n, bpc = 1000, 300
    q = _queue_without_library(typ, bpc)
    data = [np.zeros(n, np.uint8) for _ in range(3)]
    par = [np.zeros(n, np.uint8) for _ in range(2)]
    need = 5 * 4 * dl
    ro = np.zeros(need, np.uint8)
    ro.flags.writeable = False
    bad = {"dtype": np.zeros(need // 4, np.uint32), "short": np.zeros(need - 1, np.uint8), "read-only": ro,
           "not contiguous": np.zeros(2 * need, np.uint8)[::2], "not an array": bytearray(need)}
    for what, d in bad.items():
        with pytest.raises(IllegalArgumentException, match=f"digests buffer.*>= {need} bytes"):
            q.submit(data, par, digests=d)
    with pytest.raises(IllegalArgumentException, match="not both"):
        q.submit(data, par, crcs=np.zeros(20, np.uint32), digests=np.zeros(need, np.uint8))
