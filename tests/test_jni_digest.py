"""digestWindowsDirect / digestWindowsArray of jni/ozec_jni.c (OzecNative.java; HipChecksum's SHA256 / MD5 path), compiled
against the JNI test double exactly as tests/test_jni_glue.py compiles the shim, and called the way the Java classes
call them: a direct ByteBuffer or a byte[] with a position offset, a byte[] for the digests.  CPU: argument errors raise
HadoopIllegalArgumentException and leave no pin or local reference behind.  GPU: both forms and both algorithms against
hashlib, the return value being windows * digest length."""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_jni_glue import Java, P, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "ozone_amd", "lib")
vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
IAE = "org/apache/hadoop/HadoopIllegalArgumentException"
SHA256, MD5 = 4, 5


@pytest.fixture(scope="module")
def J():
    assert os.path.exists(os.path.join(LIBDIR, "libozec.so")), "libozec.so not built"
    d = tempfile.mkdtemp(prefix="ozec_mockjni_digest_")
    so = os.path.join(d, "libozec_jni_mock.so")
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "tests", "native", "mockjni"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "jni", "ozec_jni.c"), os.path.join(ROOT, "jni", "ozec_marshal.c"),
                    os.path.join(ROOT, "tests", "native", "mockjni", "mockjni.c"), "-L", LIBDIR, "-lozec",
                    "-Wl,--wrap=ozec_encode,--wrap=ozec_decode,--wrap=ozec_crc_update,--wrap=ozec_checksum_windows,"
                    "--wrap=ozec_encode_cb,--wrap=ozec_decode_cb,"
                    "--wrap=ozec_host_alloc,--wrap=ozec_host_free",
                    f"-Wl,-rpath,{LIBDIR}", "-o", so], check=True, capture_output=True, timeout=120)
    lib = ctypes.CDLL(so)
    for name, res, args in [
        ("mock_env", vp, []), ("mock_direct", vp, [vp, i64]), ("mock_heap_buffer", vp, [vp, i64]),
        ("mock_bytes", vp, [vp, i64]), ("mock_ints", vp, [vp, i64]), ("mock_objects", vp, [i64]),
        ("mock_set", None, [vp, i64, vp]), ("mock_free", None, [vp]),
        ("mock_pins", ctypes.c_int, []), ("mock_local_refs", ctypes.c_int, []),
        ("mock_take_exception", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
        (P + "digestWindowsDirect", i32, [vp, vp, i32, vp, i32, i32, i32, vp]),
        (P + "digestWindowsArray", i32, [vp, vp, i32, vp, i32, i32, i32, vp])]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.env = lib.mock_env()
    return lib


@pytest.fixture
def java(J):
    j = Java(J)
    yield j
    assert J.mock_pins() == 0, "a pinned array was not released"
    assert J.mock_local_refs() == 0, "a local reference was not deleted"
    j.close()


@pytest.mark.parametrize("fn,wrap", [("digestWindowsDirect", "direct"), ("digestWindowsArray", "bytes")])
def test_argument_errors_raise_and_release_everything(J, java, fn, wrap):
    data = np.zeros(100, np.uint8)
    out = np.full(64, 0xA5, np.uint8)
    mk = getattr(java, wrap)
    for typ in (SHA256, MD5):
        assert call(J, fn, typ, mk(data), 0, 100, 0, java.bytes(out)) == 0
        assert java.exception() == (IAE, "bytesPerChecksum must be positive")
        assert call(J, fn, typ, mk(data), 0, 100, -4, java.bytes(out)) == 0
        assert java.exception() == (IAE, "bytesPerChecksum must be positive")
        assert call(J, fn, typ, mk(data), 90, 20, 16, java.bytes(out)) == 0  # offset + length past the data
        assert java.exception()[0] == IAE
        assert call(J, fn, typ, mk(data), 0, 100, 10, java.bytes(out[:31])) == 0  # 10 windows need 320 / 160 bytes
        assert java.exception() == (IAE, "checksum output too small")
        assert call(J, fn, typ, mk(data), 0, 100, 10, None) == 0
        assert java.exception() == (IAE, "null checksum output")
        assert call(J, fn, typ, mk(data), 0, 0, 16, java.bytes(out)) == 0  # empty data: an empty list, no exception
        assert java.exception() is None
    for typ in (1, 2, 3, 6):  # NONE, the CRC types (checksumWindows*), and a value outside ChecksumType
        assert call(J, fn, typ, mk(data), 0, 100, 50, java.bytes(out)) == 0
        exc = java.exception()
        assert exc[0] == IAE and "ozec_checksum_windows" in exc[1], exc
    assert (out == 0xA5).all()
    assert J.mock_pins() == 0 and J.mock_local_refs() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("typ,name,dl", [(SHA256, "sha256", 32), (MD5, "md5", 16)])
def test_direct_and_heap_forms_vs_hashlib(J, java, typ, name, dl):
    rng = np.random.default_rng([0xD16E57, 77, typ])
    for n, bpc, pos in ((70000, 16384, 5), (1000, 100, 1), (4099, 4096, 3)):
        data = rng.integers(0, 256, n + pos + 9, dtype=np.uint8)
        nw = (n + bpc - 1) // bpc
        want = b"".join(hashlib.new(name, data[pos + o:pos + min(o + bpc, n)].tobytes()).digest()
                        for o in range(0, n, bpc))
        for fn, wrap in (("digestWindowsArray", java.bytes), ("digestWindowsDirect", java.direct)):
            out = np.full(nw * dl + 64, 0xA5, np.uint8)
            assert call(J, fn, typ, wrap(data), pos, n, bpc, java.bytes(out)) == nw * dl
            assert java.exception() is None
            assert out[:nw * dl].tobytes() == want, (fn, n, bpc)
            assert (out[nw * dl:] == 0xA5).all()
