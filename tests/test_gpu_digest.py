"""SHA256 / MD5 window digests on the GPU (digest.hip through ozec_digest_*), byte for byte against hashlib.

Reference semantics: Checksum.computeChecksum with ChecksumType SHA256 / MD5 -- one MessageDigest.digest() per
bytesPerChecksum window, the last window short (CM/Checksum.java:43-57,76-81,157-200).  One lane hashes one window, so
the cases are chosen by what a lane, a wave and a block can get wrong: every padding edge of the final block(s), lane
and block tails, full and short windows side by side in one wave, cells at any byte address and stride, the production
window sizes, verify mode's first-failure rule, the host staging pipeline and the Python API.  Outputs are pre-filled
with 0xA5 and followed by a 64-byte guard that must stay 0xA5.
"""
import ctypes
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from devcopy import to_dev, to_host  # noqa: E402
pytestmark = pytest.mark.gpu

from ozone_amd import _lib as L  # noqa: E402
from ozone_amd import checksum as ck  # noqa: E402

GUARD = 64
ALGOS = [pytest.param(ck.ChecksumType.SHA256, "sha256", 32, id="sha256"),
         pytest.param(ck.ChecksumType.MD5, "md5", 16, id="md5")]
algos = pytest.mark.parametrize("typ,name,dl", ALGOS)


def _rng(*tag):
    return np.random.default_rng([0xD16E57, *tag])


def _ref(name, cell, bpc):
    """hashlib digests of the windows of one cell, concatenated: [nwin * dl] uint8"""
    b = cell.tobytes()
    return np.frombuffer(b"".join(hashlib.new(name, b[o:o + bpc]).digest() for o in range(0, len(b), bpc)), np.uint8)


def _place(cells, base_off, slack, gap):
    """the cells at base_off + c * (n + slack) of a host image whose every other byte is `gap`"""
    n = len(cells[0])
    stride = n + slack
    img = np.full(base_off + len(cells) * stride + 16, gap, np.uint8)
    for c, cell in enumerate(cells):
        img[base_off + c * stride: base_off + c * stride + n] = cell
    return img, stride


def _device_digests(typ, dl, cells, bpc, base_off=0, slack=0, gap=0xA5):
    n = len(cells[0])
    nwin = (n + bpc - 1) // bpc
    img, stride = _place(cells, base_off, slack, gap)
    d = to_dev(img)
    out = to_dev(np.full(len(cells) * nwin * dl + GUARD, 0xA5, np.uint8))
    ck.digest_windows_batch(typ, d.data_ptr() + base_off, stride, len(cells), n, bpc, out)
    h = to_host(out)
    assert (h[-GUARD:] == 0xA5).all(), "wrote past the digests"
    return h[:-GUARD].reshape(len(cells), nwin * dl)


def _check(typ, name, dl, cells, bpc, **kw):
    got = _device_digests(typ, dl, cells, bpc, **kw)
    for c, cell in enumerate(cells):
        want = _ref(name, cell, bpc)
        bad = np.flatnonzero((got[c] != want).reshape(-1, dl).any(axis=1))
        assert bad.size == 0, (name, len(cell), bpc, kw, "cell", c, "windows", bad[:8].tolist())
    return got


@algos
def test_padding_edges(typ, name, dl):
    """one window per cell, bpc = len = N across every boundary of the one- and two-block padding"""
    r = _rng(1)
    for n in (1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129):
        _check(typ, name, dl, [r.integers(0, 256, n, dtype=np.uint8) for _ in range(3)], n)


@algos
@pytest.mark.parametrize("bpc", [64, 100])
def test_lane_and_block_tails(typ, name, dl, bpc):
    """window counts around the wave (64 lanes) and the block (256 threads); bpc = 64 has no tail bytes, 100 has 36"""
    r = _rng(2, bpc)
    for nwin in (1, 63, 64, 65, 255, 256, 257):
        _check(typ, name, dl, [r.integers(0, 256, nwin * bpc, dtype=np.uint8)], bpc)


@algos
@pytest.mark.parametrize("last", [1, 55, 56, 64])
def test_full_and_short_windows_in_one_wave(typ, name, dl, last):
    """5 cells x 13 windows of bpc = 100: 65 units that cross cell boundaries and two waves, every 13th window short"""
    r = _rng(3, last)
    _check(typ, name, dl, [r.integers(0, 256, 12 * 100 + last, dtype=np.uint8) for _ in range(5)], 100)


@algos
def test_placement_any_address_any_stride(typ, name, dl):
    """base address off by 1, 3, 7, 15 bytes; cell_stride = len + 0, 1, 33; the bytes between and around the cells are
    then changed and the call repeated: the digests must not move (nothing outside [cell, cell + len) is hashed)"""
    r = _rng(4)
    n, bpc = 1000 + 37, 300  # windows of 4 blocks + 44 bytes, a last window of 137 bytes
    cells = [r.integers(0, 256, n, dtype=np.uint8) for _ in range(4)]
    for off in (1, 3, 7, 15):
        for slack in (0, 1, 33):
            a = _check(typ, name, dl, cells, bpc, base_off=off, slack=slack, gap=0xA5)
            b = _check(typ, name, dl, cells, bpc, base_off=off, slack=slack, gap=0x3C)
            assert (a == b).all(), (off, slack)


@algos
def test_production_window_sizes(typ, name, dl):
    r = _rng(5)
    _check(typ, name, dl, [r.integers(0, 256, 65536 + 700, dtype=np.uint8) for _ in range(2)], 16384)
    _check(typ, name, dl, [r.integers(0, 256, (1 << 20) + 1, dtype=np.uint8)], 1 << 20)


@algos
def test_verify_batch_reports_first_failing_window(typ, name, dl):
    r = _rng(6)
    ncells, nwin, bpc = 6, 70, 100  # 420 units: two blocks, windows of one block + 36 bytes, last window 57 bytes
    n = (nwin - 1) * bpc + 57
    cells = [r.integers(0, 256, n, dtype=np.uint8) for _ in range(ncells)]
    expected = np.stack([_ref(name, c, bpc) for c in cells])  # [ncells][nwin * dl], from hashlib
    data = np.stack(cells)

    def verify(dat, exp, off=0):
        img, stride = _place(list(dat), off, 5, 0xA5)
        d = to_dev(img)
        e = to_dev(exp)
        mis = to_dev(np.full(ncells + 16, 0x5A5A5A5A, np.int32))
        ck.digest_verify_batch(typ, d.data_ptr() + off, stride, ncells, n, bpc, e, mis)
        m = to_host(mis)
        assert (m[ncells:] == 0x5A5A5A5A).all()
        return m[:ncells].tolist()

    assert verify(data, expected) == [-1] * ncells
    bad = data.copy()
    exp = expected.copy()
    bad[1, 37 * bpc + 99] ^= 0x01          # cell 1: one data byte in window 37
    exp[3, 5 * dl + dl - 1] ^= 0x80        # cell 3: the last byte of window 5's stored digest
    bad[4, 69 * bpc + 56] ^= 0x10          # cell 4: the last byte of the short last window ...
    bad[4, 12 * bpc] ^= 0xFF               # ... and window 12: the first failure is reported
    assert verify(bad, exp, off=3) == [-1, 37, -1, 5, 12, -1]


def _host_digests(typ, dl, src_addr, n, bpc, out_arr):
    rc = L.lib().ozec_digest_windows(int(typ), src_addr, n, bpc, out_arr.ctypes.data)
    assert rc == L.OZEC_OK, L.last_error()


@algos
def test_host_form_pageable_pinned_registered(typ, name, dl):
    """ozec_digest_windows through the staging pipeline.  Length: staged_pipeline (capi.cpp) cuts a pageable call into
    chunks of host_chunk bytes (read here with ozec_get_tuning) rounded down to whole groups of windows of at least
    4096 bytes -- bpc = 1000 gives 5000 -- so two such chunks plus three windows plus 17 bytes make three chunks, the
    last ending in a 17-byte window."""
    from ozone_amd.stripe_queue import host_alloc, host_register, host_unregister
    lib = L.lib()
    bpc = 1000
    hc = ctypes.c_int64(0)
    assert lib.ozec_get_tuning(b"host_chunk", ctypes.byref(hc)) == 0 and hc.value >= 5000
    gran = (4096 + bpc - 1) // bpc * bpc
    chunk = hc.value // gran * gran
    n = 2 * chunk + 3 * bpc + 17
    assert (n + chunk - 1) // chunk == 3
    r = _rng(7)
    data = r.integers(0, 256, n, dtype=np.uint8)
    want = _ref(name, data, bpc)
    nout = want.size
    # pageable in and out
    out = np.full(nout + GUARD, 0xA5, np.uint8)
    _host_digests(typ, dl, data.ctypes.data, n, bpc, out)
    assert (out[:nout] == want).all() and (out[nout:] == 0xA5).all()
    small = np.full(dl + GUARD, 0xA5, np.uint8)
    _host_digests(typ, dl, data.ctypes.data, 100, bpc, small)  # one short window
    assert small[:dl].tobytes() == hashlib.new(name, data[:100].tobytes()).digest() and (small[dl:] == 0xA5).all()
    # input and output in one pinned allocation, at odd offsets
    pool = host_alloc(n + nout + GUARD + 256)
    src = pool.array[3:3 + n]
    src[:] = data
    dst = pool.array[n + 64 + 5: n + 64 + 5 + nout + GUARD]
    dst[:] = 0xA5
    _host_digests(typ, dl, src.ctypes.data, n, bpc, dst)
    assert (dst[:nout] == want).all() and (dst[nout:] == 0xA5).all()
    dst[:] = 0xA5
    _host_digests(typ, dl, src.ctypes.data, 100, bpc, dst)
    assert dst[:dl].tobytes() == hashlib.new(name, data[:100].tobytes()).digest() and (dst[dl:] == 0xA5).all()
    del src, dst
    pool.free()
    # a caller's own buffer, registered
    page = 4096
    buf = np.zeros(n + nout + GUARD + 3 * page, np.uint8)
    base = (-buf.ctypes.data) % page
    span = (n + nout + GUARD + 64 + page - 1) // page * page
    host_register(buf.ctypes.data + base, span, -1)
    try:
        src = buf[base + 1: base + 1 + n]
        src[:] = data
        dst = buf[base + n + 32: base + n + 32 + nout + GUARD]
        dst[:] = 0xA5
        _host_digests(typ, dl, src.ctypes.data, n, bpc, dst)
        assert (dst[:nout] == want).all() and (dst[nout:] == 0xA5).all()
    finally:
        host_unregister(buf.ctypes.data + base)
    del src, dst, buf


@algos
def test_python_checksum_api(typ, name, dl):
    r = _rng(8)
    bpc = 4096
    data = r.integers(0, 256, 10 * bpc + 123, dtype=np.uint8)
    want = [hashlib.new(name, data[o:o + bpc].tobytes()).digest() for o in range(0, data.size, bpc)]
    assert ck.digest_windows(typ, data, bpc) == want
    cd = ck.Checksum(typ, bpc).compute_checksum(data)
    assert cd.get_checksum_type() == typ and cd.get_bytes_per_checksum() == bpc
    assert cd.get_checksums() == want and all(len(x) == dl for x in cd.get_checksums())
    # ChecksumData round trip: what compute_checksum returned verifies, and equals a ChecksumData built from hashlib
    assert cd == ck.ChecksumData(typ, bpc, want)
    assert ck.Checksum.verify_checksum(data, cd)
    assert ck.Checksum.verify_checksum(data, ck.ChecksumData(typ, bpc, list(cd.get_checksums())))
    bad = data.copy()
    bad[7 * bpc + 5] ^= 1
    with pytest.raises(ck.OzoneChecksumException) as ei:
        ck.Checksum.verify_checksum(bad, cd)
    assert ei.value.index == 7 and str(ei.value) == "Checksum mismatch at index 7"
    # start_index: the stored list holds two earlier windows (ChecksumData.verifyChecksumDataMatches)
    shifted = ck.ChecksumData(typ, bpc, [b"\0" * dl, b"\1" * dl] + want)
    assert ck.Checksum.verify_checksum(data, shifted, 2)
    with pytest.raises(ck.OzoneChecksumException) as ei:
        ck.Checksum.verify_checksum(data, shifted, 1)
    assert ei.value.index == 0


@pytest.mark.parametrize("i", range(200))
def test_random_sweep(i):
    """seeded draws over algorithm, 1-9 cells, len 1-5000, bpc 1-700, base offset 0-15, stride slack 0-33"""
    r = _rng(9, i)
    typ, name, dl = [(ck.ChecksumType.SHA256, "sha256", 32), (ck.ChecksumType.MD5, "md5", 16)][int(r.integers(0, 2))]
    ncells = int(r.integers(1, 10))
    n = int(r.integers(1, 5001))
    bpc = int(r.integers(1, 701))
    off = int(r.integers(0, 16))
    slack = int(r.integers(0, 34))
    _check(typ, name, dl, [r.integers(0, 256, n, dtype=np.uint8) for _ in range(ncells)], bpc, base_off=off,
           slack=slack, gap=int(r.integers(0, 256)))
