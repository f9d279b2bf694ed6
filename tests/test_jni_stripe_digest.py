"""queueCreate / queueSubmit and reconstructHostBatch of jni/ozec_jni.c with ChecksumType SHA256 (4) and MD5 (5), through
the JNI test double of tests/test_jni_glue.py and called the way HipStripeQueue and AbstractHipRawDecoder call them.  The
native signatures are those of the CRC types; the marshal layer (jni/ozec_marshal.c) sizes the checksum buffers with
the digest length and calls ozec_stripe_queue_submit_digests / ozec_reconstruct_digest_host_batch.  Digests against
hashlib, parity and rebuilt units against the oracle; a digest buffer one byte short raises
HadoopIllegalArgumentException and leaves no pin or local reference behind (the `java` fixture checks both)."""
import ctypes
import hashlib

import numpy as np
import pytest

import oracle
from test_jni_glue import J, call, java  # noqa: F401  (J and java are fixtures)

pytestmark = pytest.mark.gpu
IAE = "org/apache/hadoop/HadoopIllegalArgumentException"
ALGOS = [(4, "sha256", 32), (5, "md5", 16)]
algos = pytest.mark.parametrize("typ,name,dl", ALGOS, ids=[a[1] for a in ALGOS])


def _digests(name, unit, bpc):
    b = np.ascontiguousarray(unit).tobytes()
    return np.stack([np.frombuffer(hashlib.new(name, b[o:o + bpc]).digest(), np.uint8) for o in range(0, len(b), bpc)])


@algos
def test_stripe_queue_digests_through_jni(J, java, typ, name, dl):  # noqa: F811
    k, p, n, bpc = 6, 3, 1037, 300
    nwin = -(-n // bpc)
    need = (k + p) * nwin * dl
    rng = np.random.default_rng([typ, 31])
    h = call(J, "coderCreate", 0, 0, k, p)
    q = call(J, "queueCreate", h, n, 2, typ, bpc)
    assert java.exception() is None and q
    jobs = []

    def submit(d, par, buf, off):
        return call(J, "queueSubmit", q, java.array([java.direct(x) for x in d]), java.ints([0] * k),
                    java.array([java.direct(x) for x in par]), java.ints([0] * p), n, java.direct(buf), off)
    try:
        d = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(k)]
        par = [np.full(n, 0xA5, np.uint8) for _ in range(p)]
        submit(d, par, np.zeros(need - 1, np.uint8), 0)  # one byte short
        ex = java.exception()
        assert ex[0] == IAE and "too small" in ex[1], ex
        submit(d, par, np.zeros(need + 8, np.uint8), 9)  # the position leaves it one byte short
        ex = java.exception()
        assert ex[0] == IAE and "too small" in ex[1], ex
        assert J.mock_pins() == 0 and J.mock_local_refs() == 0
        for s in range(3):  # a full batch and a partial one
            d = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(k)]
            par = [np.full(n, 0xA5, np.uint8) for _ in range(p)]
            buf = np.full(7 + need + 64, 0xA5, np.uint8)
            t = submit(d, par, buf, 7)
            assert java.exception() is None
            jobs.append((t, d, par, buf))
        call(J, "queueWait", q, jobs[-1][0])
        assert java.exception() is None
        for t, d, par, buf in jobs:
            ref = oracle.rs_encode(k, p, d)
            assert all((par[r] == ref[r]).all() for r in range(p)), t
            want = np.stack([_digests(name, u, bpc) for u in d + ref])
            assert (buf[7:7 + need].reshape(k + p, nwin, dl) == want).all(), t
            assert (buf[:7] == 0xA5).all() and (buf[7 + need:] == 0xA5).all(), t
    finally:
        call(J, "queueFree", q)
        call(J, "coderRelease", h)
    assert java.exception() is None


@algos
def test_reconstruct_batch_digests_through_jni(J, java, typ, name, dl):  # noqa: F811
    k, p, n, S, bpc = 6, 3, 1037, 3, 300
    nwin = -(-n // bpc)
    erased = [0, 2, 7]
    e = len(erased)
    present = [u for u in range(k + p) if u not in erased]
    rng = np.random.default_rng([typ, 32])
    h = call(J, "coderCreate", 1, 0, k, p)
    pbs = []
    try:
        def pinned(nbytes):
            pb = call(J, "allocatePinned", nbytes)
            assert java.exception() is None and pb
            pbs.append(pb)
            return pb, np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(J.mock_data(pb)))
        sb, sv = pinned(S * (k + p) * n)
        eb, ev = pinned(S * (k + p) * nwin * dl)
        ob, ov = pinned(S * e * n)
        cb, cv = pinned(S * e * nwin * dl)
        mb, mv = pinned(S * 4)
        stripes = sv.reshape(S, k + p, n)
        for s in range(S):
            d = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(k)]
            for u, x in enumerate(d + oracle.rs_encode(k, p, d)):
                stripes[s, u] = x
        orig = stripes.copy()
        dig = np.stack([np.stack([_digests(name, orig[s, u], bpc) for u in range(k + p)]) for s in range(S)])
        ev[:] = dig.reshape(-1)
        args = (h, sb, (k + p) * n, n, java.ints(present), java.ints(erased), ob, S, n, typ, bpc)
        short = java.direct(np.zeros(S * e * nwin * dl - 1, np.uint8))
        call(J, "reconstructHostBatch", *args, eb, short, mb)
        ex = java.exception()
        assert ex[0] == IAE and "checksum output buffer too small" in ex[1], ex
        short = java.direct(np.zeros(S * (k + p) * nwin * dl - 1, np.uint8))
        call(J, "reconstructHostBatch", *args, short, cb, mb)
        ex = java.exception()
        assert ex[0] == IAE and "expected checksum buffer too small" in ex[1], ex
        assert J.mock_pins() == 0 and J.mock_local_refs() == 0
        stripes[:, erased] = 0xEE
        stripes[1, present[k - 1], bpc + 3] ^= 0x80  # stripe 1: the last unit read is corrupted in window 1
        cv[:] = 0xA5
        mv.view(np.int32)[:] = 0x5A5A5A5A
        call(J, "reconstructHostBatch", *args, eb, cb, mb)
        assert java.exception() is None
        got, od, mism = ov.reshape(S, e, n), cv.reshape(S, e, nwin, dl), mv.view(np.int32)
        assert list(mism) == [-1, present[k - 1] * nwin + 1, -1]
        for s in (0, 2):
            assert (got[s] == orig[s, erased]).all() and (od[s] == dig[s, erased]).all(), s
        for i in range(e):
            assert (od[1, i] == _digests(name, got[1, i], bpc)).all()
    finally:
        for pb in pbs:
            call(J, "freePinned", pb)
            J.mock_free(pb)
        call(J, "coderRelease", h)
    assert java.exception() is None
