"""Stripes coded and checksummed with ChecksumType SHA256 / MD5 in one call (GPU): ozec_encode_digest_batch,
ozec_reconstruct_digest_batch, their host-batch forms and the stripe queue's digest submit.

Expected digests come from hashlib (MessageDigest per bytesPerChecksum window, Checksum.java:43-57,76-81), expected
parity and rebuilt units from the oracle (RSUtil.encodeData, XORRawEncoder); nothing is compared with the code under
test.  Digest and mismatch buffers are pre-filled with 0xA5 / 0x5A5A5A5A and followed by a guard that must survive.
Shapes are the smallest that can still go wrong: one wave that mixes stripes, data and parity units of two allocations;
short last windows; MD5 on both sides of its 256-byte cooperative threshold; cells at odd addresses with stride slack;
units more than 2 GiB apart."""
import ctypes
import hashlib

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
from devcopy import to_dev, to_host  # noqa: E402
pytestmark = pytest.mark.gpu

from ozone_amd import _lib as L  # noqa: E402
from ozone_amd import rawcoder as rc  # noqa: E402
from ozone_amd.checksum import ChecksumType  # noqa: E402
from ozone_amd.stripe_queue import StripeQueue, host_alloc, host_register, host_unregister  # noqa: E402

DEV = "cuda:0"
GUARD = 64
ALGOS = [(4, "sha256", 32), (5, "md5", 16)]
algos = pytest.mark.parametrize("typ,name,dl", ALGOS, ids=[a[1] for a in ALGOS])
CODECS = [("rs", 3, 2), ("rs", 6, 3), ("xor", 2, 1), ("xor", 3, 2)]


def _digests(name, unit, bpc):
    """hashlib digest of every bpc-window of `unit` -> uint8 [nwin][digest length]"""
    b = np.ascontiguousarray(unit).tobytes()
    return np.stack([np.frombuffer(hashlib.new(name, b[o:o + bpc]).digest(), np.uint8) for o in range(0, len(b), bpc)])


def _coded(codec, k, p, data):
    """the coded parity rows of one stripe (XOR: one) from the oracle"""
    return [oracle.xor_encode(list(data))] if codec == "xor" else oracle.rs_encode(k, p, list(data))


_REF = {}


def _reference(codec, k, p, S, n, bpc, seed):
    """data [S][k][n], coded rows [S][rows][n] and, per algorithm, digests [S][k+rows][nwin][dl]; computed once per
    shape and shared, never changed"""
    key = (codec, k, p, S, n, bpc, seed)
    if key not in _REF:
        rng = np.random.default_rng([k, p, S, n, bpc, seed])
        data = rng.integers(0, 256, (S, k, n), dtype=np.uint8)
        coded = np.stack([np.stack(_coded(codec, k, p, data[s])) for s in range(S)])
        units = np.concatenate([data, coded], axis=1)
        dig = {name: np.stack([np.stack([_digests(name, u, bpc) for u in units[s]]) for s in range(S)])
               for _, name, _ in ALGOS}
        for a in (data, coded, units, *dig.values()):
            a.flags.writeable = False
        _REF[key] = (data, coded, units, dig)
    return _REF[key]


def _encode_case(codec, k, p, S, n, bpc, in_off, out_off, slack, typ, name, dl, seed=0):
    data, coded, _, dig = _reference(codec, k, p, S, n, bpc, seed)
    rows = coded.shape[1]
    nwin = -(-n // bpc)
    us = n + slack
    in_ss, out_ss = k * us + slack, p * us + 2 * slack
    in_bytes, out_bytes = in_off + S * in_ss + GUARD, out_off + S * out_ss + GUARD
    nd = S * (k + rows) * nwin * dl
    enc = rc.RawErasureEncoder(rc.ECReplicationConfig(k, p, codec))
    results = []
    for fill in (0x11, 0xC7):  # the bytes between and around the cells differ between the two passes
        hin = np.full(in_bytes, fill, np.uint8)
        for s in range(S):
            for j in range(k):
                o = in_off + s * in_ss + j * us
                hin[o:o + n] = data[s, j]
        d_in = to_dev(hin)
        d_out = to_dev(np.full(out_bytes, fill ^ 0xFF, np.uint8))
        d_dig = to_dev(np.full(nd + GUARD, 0xA5, np.uint8))
        enc.encode_digest_batch(d_in[in_off:], in_ss, us, d_out[out_off:], out_ss, us, S, n, typ, bpc, d_dig)
        hout, hdig = to_host(d_out), to_host(d_dig)
        assert (to_host(d_in) == hin).all(), "input modified"
        assert (hdig[nd:] == 0xA5).all(), "digest guard overwritten"
        got = hdig[:nd].reshape(S, k + rows, nwin, dl)
        mask = np.ones(out_bytes, bool)
        for s in range(S):
            for r in range(p):
                o = out_off + s * out_ss + r * us
                want = coded[s, r] if r < rows else np.zeros(n, np.uint8)  # XOR with p > 1 zero-fills the others
                assert (hout[o:o + n] == want).all(), (codec, k, p, n, bpc, s, r)
                mask[o:o + n] = False
        assert (hout[mask] == fill ^ 0xFF).all(), "bytes outside the parity cells were written"
        bad = np.argwhere((got != dig[name]).any(axis=3))
        assert bad.size == 0, (codec, k, p, n, bpc, name, "first wrong (stripe, unit, window):", bad[:3].tolist())
        results.append(got.copy())
    assert (results[0] == results[1]).all()


@algos
@pytest.mark.parametrize("codec,k,p", CODECS)
@pytest.mark.parametrize("S,n,bpc", [(3, 457, 100), (3, 1037, 300), (2, 65536 + 700, 16384)])
def test_encode_digest_batch(codec, k, p, S, n, bpc, typ, name, dl):
    for in_off, out_off, slack in ((1, 3, 0), (15, 1, 33), (3, 15, 33)):
        _encode_case(codec, k, p, S, n, bpc, in_off, out_off, slack, typ, name, dl)


@pytest.mark.parametrize("part", range(8))
def test_encode_digest_batch_seeded_sweep(part):
    """200 seeded draws, 25 per case: k 2-10, p 1-4, len 1-5000, bpc 1-700, S 1-5"""
    for i in range(25 * part, 25 * part + 25):
        r = np.random.default_rng([0xD16E57, i])
        k, p = int(r.integers(2, 11)), int(r.integers(1, 5))
        n, bpc, S = int(r.integers(1, 5001)), int(r.integers(1, 701)), int(r.integers(1, 6))
        codec = "xor" if r.integers(0, 4) == 0 else "rs"
        typ, name, dl = ALGOS[int(r.integers(0, 2))]
        nwin = -(-n // bpc)
        _, coded, _, dig = _reference(codec, k, p, S, n, bpc, i)
        rows = coded.shape[1]
        data = _reference(codec, k, p, S, n, bpc, i)[0]
        in_off, out_off, slack = int(r.integers(0, 16)), int(r.integers(0, 16)), int(r.integers(0, 40))
        us = n + slack
        hin = r.integers(0, 256, in_off + S * k * us + GUARD, dtype=np.uint8)
        for s in range(S):
            for j in range(k):
                o = in_off + (s * k + j) * us
                hin[o:o + n] = data[s, j]
        d_in = to_dev(hin)
        d_out = to_dev(np.full(out_off + S * p * us + GUARD, 0x3C, np.uint8))
        nd = S * (k + rows) * nwin * dl
        d_dig = to_dev(np.full(nd + GUARD, 0xA5, np.uint8))
        rc.RawErasureEncoder(rc.ECReplicationConfig(k, p, codec)).encode_digest_batch(
            d_in[in_off:], k * us, us, d_out[out_off:], p * us, us, S, n, typ, bpc, d_dig)
        hout, hdig = to_host(d_out), to_host(d_dig)
        case = (i, codec, k, p, n, bpc, S, name, in_off, out_off, slack)
        assert (hdig[nd:] == 0xA5).all(), case
        assert (hdig[:nd].reshape(S, k + rows, nwin, dl) == dig[name]).all(), case
        for s in range(S):
            for q in range(p):
                o = out_off + (s * p + q) * us
                assert (hout[o:o + n] == (coded[s, q] if q < rows else 0)).all(), case
                assert (hout[o + n:o + us] == 0x3C).all(), case
        assert (hout[:out_off] == 0x3C).all() and (hout[out_off + S * p * us:] == 0x3C).all(), case


@pytest.mark.parametrize("codec,k,p", [("xor", 2, 1), ("rs", 4, 2)])
def test_units_more_than_2gib_apart(codec, k, p):
    """unit stride 768 MiB, stripes side by side inside each unit slot, odd base: the 64-bit strides of the unit table"""
    US, S, n, bpc, shift = 768 << 20, 2, 65536 + 5, 16384, 3
    ss = n + 4096 + shift
    data, coded, units, dig = _reference(codec, k, p, S, n, bpc, 2)
    nwin = -(-n // bpc)
    buf = torch.empty(shift + (k + p - 1) * US + (S - 1) * ss + n + GUARD, dtype=torch.uint8, device=DEV)
    base = buf[shift:]

    def at(s, u):
        return base[s * ss + u * US:s * ss + u * US + n + 16]
    for s in range(S):
        for u in range(k + p):
            at(s, u).fill_(0x3C)
            if u < k:
                at(s, u)[:n].copy_(to_dev(data[s, u]))
    conf = rc.ECReplicationConfig(k, p, codec)
    erased = [0] if codec == "xor" else [0, k]
    present = [u for u in range(k + p) if u not in erased][:k]
    for typ, name, dl in ALGOS:
        nd = S * (k + p) * nwin * dl
        d_dig = to_dev(np.full(nd + GUARD, 0xA5, np.uint8))
        rc.RawErasureEncoder(conf).encode_digest_batch(base, ss, US, base[k * US:], ss, US, S, n, typ, bpc, d_dig)
        hdig = to_host(d_dig)
        assert (hdig[nd:] == 0xA5).all()
        assert (hdig[:nd].reshape(S, k + p, nwin, dl) == dig[name]).all(), (codec, name)
        for s in range(S):
            for q in range(p):
                cell = to_host(at(s, k + q))
                assert (cell[:n] == coded[s, q]).all() and (cell[n:] == 0x3C).all(), (codec, s, q)
        e = len(erased)
        d_out = to_dev(np.full(S * e * n + GUARD, 0x11, np.uint8))
        nod = S * e * nwin * dl
        d_od = to_dev(np.full(nod + GUARD, 0xA5, np.uint8))
        mism = to_dev(np.full(S + 4, 0x5A5A5A5A, np.int32))
        rc.RawErasureDecoder(conf).reconstruct_digest_batch(base, ss, US, present, erased, d_out, e * n, n, S, n, typ,
                                                            bpc, d_od, d_expected=d_dig, d_mismatch=mism)
        ho, hod, m = to_host(d_out), to_host(d_od), to_host(mism)
        assert (m[:S] == -1).all() and (m[S:] == 0x5A5A5A5A).all(), m
        assert (ho[S * e * n:] == 0x11).all() and (hod[nod:] == 0xA5).all()
        for s in range(S):
            for i, u in enumerate(erased):
                assert (ho[(s * e + i) * n:(s * e + i + 1) * n] == units[s, u]).all(), (codec, s, u)
        assert (hod[:nod].reshape(S, e, nwin, dl) == dig[name][:, erased]).all()
    del buf, base


REC = [("rs", 6, 3, [0, 2, 7]), ("rs", 6, 3, [1]), ("rs", 10, 4, [0, 1, 2, 3]), ("rs", 10, 4, [1, 4, 10, 13]),
       ("rs", 3, 2, [4]), ("xor", 2, 1, [1])]


def _rec_setup(codec, k, p, erased, n, bpc, name, dl):
    """4 stripes: erased units 0xEE in the input, unread units' stored digests garbage, stripe 1 corrupted in
    (read[-1], window 1) and (read[0], window 2), stripe 2 with one flipped byte in a stored digest"""
    S = 4
    _, _, units, dig = _reference(codec, k, p, S, n, bpc, 1)
    nwin = -(-n // bpc)
    read = [u for u in range(k + p) if u not in erased][:k]
    inp = units.copy()
    inp[:, erased] = 0xEE
    inp[1, read[-1], bpc + 1] ^= 0x10
    inp[1, read[0], 2 * bpc + 5] ^= 0x01
    stored = dig[name].copy()
    for u in range(k + p):
        if u not in read:
            stored[:, u] = 0x77
    stored[2, read[1 % k], 0, dl - 1] ^= 0x80
    want_m = [-1, read[0] * nwin + 2, read[1 % k] * nwin, -1]
    return S, units, dig[name], nwin, read, inp, stored, want_m


def _rec_check(out, odig, m, S, units, dig, erased, bpc, name, want_m, case):
    assert m.tolist() == want_m, (case, m)
    for s in range(S):
        for i, e in enumerate(erased):
            if want_m[s] == -1 or s == 2:  # clean input: exact units, hashlib's digests of the original units
                assert (out[s, i] == units[s, e]).all(), (case, s, e)
                assert (odig[s, i] == dig[s, e]).all(), (case, s, e)
            else:  # the corrupted stripe's digests describe what was written
                assert (odig[s, i] == _digests(name, out[s, i], bpc)).all(), (case, s, e)


@algos
@pytest.mark.parametrize("codec,k,p,erased", REC, ids=[f"{c}-{k}-{p}-{'_'.join(map(str, e))}" for c, k, p, e in REC])
@pytest.mark.parametrize("n,bpc", [(1037, 300), (1 << 16, 16384)])
def test_reconstruct_digest_batch(codec, k, p, erased, n, bpc, typ, name, dl):
    S, units, dig, nwin, read, inp, stored, want_m = _rec_setup(codec, k, p, erased, n, bpc, name, dl)
    e, off = len(erased), 1
    present = [u for u in range(k + p) if u not in erased]
    hin = np.concatenate([np.full(off, 0x42, np.uint8), inp.reshape(-1), np.full(GUARD, 0x42, np.uint8)])
    d_in = to_dev(hin)
    ous, oss = n + 33, e * (n + 33) + 7
    nod = S * e * nwin * dl
    dec = rc.RawErasureDecoder(rc.ECReplicationConfig(k, p, codec))
    case = (codec, k, p, erased, n, bpc, name)
    for d_exp in (to_dev(stored.reshape(-1)), None):
        d_out = to_dev(np.full(3 + S * oss + GUARD, 0x11, np.uint8))
        d_od = to_dev(np.full(nod + GUARD, 0xA5, np.uint8))
        mism = to_dev(np.full(S + 4, 0x5A5A5A5A, np.int32))
        dec.reconstruct_digest_batch(d_in[off:], (k + p) * n, n, present, erased, d_out[3:], oss, ous, S, n, typ, bpc,
                                     d_od, d_expected=d_exp, d_mismatch=mism)
        ho, hod, m = to_host(d_out), to_host(d_od), to_host(mism)
        assert (to_host(d_in) == hin).all(), "input modified"
        assert (hod[nod:] == 0xA5).all() and (m[S:] == 0x5A5A5A5A).all(), case
        out = np.stack([np.stack([ho[3 + s * oss + i * ous:3 + s * oss + i * ous + n] for i in range(e)])
                        for s in range(S)])
        mask = np.ones(ho.size, bool)
        for s in range(S):
            for i in range(e):
                mask[3 + s * oss + i * ous:3 + s * oss + i * ous + n] = False
        assert (ho[mask] == 0x11).all(), "bytes outside the rebuilt cells were written"
        if d_exp is None:  # no verification: -1 everywhere, the outputs the same
            want = [-1] * S
            assert m[:S].tolist() == want, (case, m)
            for s in range(S):
                for i in range(e):
                    assert (hod[:nod].reshape(S, e, nwin, dl)[s, i] == _digests(name, out[s, i], bpc)).all(), (case, s)
            for s in (0, 2, 3):
                assert (out[s] == units[s, erased]).all(), (case, s)
        else:
            _rec_check(out, hod[:nod].reshape(S, e, nwin, dl), m[:S], S, units, dig, erased, bpc, name, want_m, case)


@algos
def test_xor_decoder_zero_filled_outputs_get_digests(typ, name, dl):
    """xor-3-2 asked for two units: only the first is rebuilt (from every other unit, the all-zero second parity
    included, XORRawDecoder.java:40-86), the second output is zero-filled, and both have digests"""
    k, p, S, n, bpc, erased = 3, 2, 2, 457, 100, [1, 4]
    _, _, units, dig = _reference("xor", k, p, S, n, bpc, 3)
    nwin = -(-n // bpc)
    inp = np.zeros((S, k + p, n), np.uint8)
    inp[:, :k + 1] = units
    inp[:, 1] = 0xEE
    d_out = to_dev(np.full(S * 2 * n + GUARD, 0x11, np.uint8))
    nod = S * 2 * nwin * dl
    d_od = to_dev(np.full(nod + GUARD, 0xA5, np.uint8))
    dec = rc.RawErasureDecoder(rc.ECReplicationConfig(k, p, "xor"))
    dec.reconstruct_digest_batch(to_dev(inp), (k + p) * n, n, [0, 2, 3, 4], erased, d_out, 2 * n, n, S, n, typ, bpc, d_od)
    ho, hod = to_host(d_out), to_host(d_od)
    assert (ho[S * 2 * n:] == 0x11).all() and (hod[nod:] == 0xA5).all()
    out, od = ho[:S * 2 * n].reshape(S, 2, n), hod[:nod].reshape(S, 2, nwin, dl)
    zero = _digests(name, np.zeros(n, np.uint8), bpc)
    for s in range(S):
        assert (out[s, 0] == units[s, 1]).all() and (out[s, 1] == 0).all()
        assert (od[s, 0] == dig[name][s, 1]).all() and (od[s, 1] == zero).all()


# ---- host batches -----------------------------------------------------------------------------------------------------

@pytest.fixture
def device_list():
    yield rc.set_devices
    rc.set_devices(None)


class _HostMem:
    """byte ranges of one kind of host memory: pageable, pinned (ozec_host_alloc) or registered"""

    def __init__(self, kind, nbytes):
        self.kind, page = kind, 4096
        if kind == "pinned":
            self.pool = host_alloc(nbytes + 64)
            self.mem = self.pool.array[5:5 + nbytes]
        elif kind == "registered":
            self.raw = np.zeros(nbytes + 3 * page, np.uint8)
            base = (-self.raw.ctypes.data) % page
            self.addr = self.raw.ctypes.data + base
            host_register(self.addr, (nbytes + 64 + page - 1) // page * page, -1)
            self.mem = self.raw[base + 1:base + 1 + nbytes]
        else:
            self.mem = np.zeros(nbytes, np.uint8)

    def close(self):
        self.mem = None
        if self.kind == "pinned":
            self.pool.free()
        elif self.kind == "registered":
            host_unregister(self.addr)


def _carve(mem, sizes):
    out, o = [], 0
    for n in sizes:
        out.append(mem[o:o + n])
        o += n + 3  # odd spacing
    return out


@algos
@pytest.mark.parametrize("codec,k,p", [("rs", 3, 2), ("xor", 3, 2)])
@pytest.mark.parametrize("kind", ["pageable", "pinned", "registered", "two-devices"])
def test_encode_digest_host_batch(codec, k, p, kind, typ, name, dl, device_list):
    S, n, bpc = 5, 1037, 300  # stripes_per_chunk = 2: three chunks, the last short
    data, coded, _, dig = _reference(codec, k, p, S, n, bpc, 4)
    rows, nwin = coded.shape[1], -(-n // bpc)
    if kind == "two-devices":
        device_list([0, 0])
    nd = S * (k + rows) * nwin * dl
    hm = _HostMem("pageable" if kind == "two-devices" else kind, S * (k + p) * n + nd + 2 * GUARD + 64)
    try:
        h_in, h_out, h_dig = _carve(hm.mem, [S * k * n, S * p * n + GUARD, nd + GUARD])
        h_in[:] = data.reshape(-1)
        h_out[:] = 0x11
        h_dig[:] = 0xA5
        enc = rc.RawErasureEncoder(rc.ECReplicationConfig(k, p, codec))
        enc.encode_digest_host_batch(h_in, k * n, n, h_out, p * n, n, S, n, typ, bpc, h_dig, stripes_per_chunk=2)
        assert (h_in == data.reshape(-1)).all()
        assert (h_out[S * p * n:] == 0x11).all() and (h_dig[nd:] == 0xA5).all()
        par = h_out[:S * p * n].reshape(S, p, n)
        assert (par[:, :rows] == coded).all() and (par[:, rows:] == 0).all(), (codec, kind)
        assert (h_dig[:nd].reshape(S, k + rows, nwin, dl) == dig[name]).all(), (codec, kind, name)
        del h_in, h_out, h_dig, par
    finally:
        hm.close()


@algos
@pytest.mark.parametrize("codec,k,p,erased", [("rs", 6, 3, [0, 2, 7]), ("xor", 2, 1, [1])])
@pytest.mark.parametrize("kind", ["pageable", "pinned", "registered", "two-devices"])
def test_reconstruct_digest_host_batch(codec, k, p, erased, kind, typ, name, dl, device_list):
    n, bpc = 1037, 300
    S4, units4, dig4, nwin, read, inp4, stored4, want4 = _rec_setup(codec, k, p, erased, n, bpc, name, dl)
    # a fifth, clean stripe (a copy of stripe 0): S = 5 with stripes_per_chunk = 2 is three chunks, the last short
    S = 5
    units, dig = np.concatenate([units4, units4[:1]]), np.concatenate([dig4, dig4[:1]])
    inp, stored, want_m = np.concatenate([inp4, inp4[:1]]), np.concatenate([stored4, stored4[:1]]), want4 + [-1]
    if kind == "two-devices":
        device_list([0, 0])
    e = len(erased)
    present = [u for u in range(k + p) if u not in erased]
    nod, nex = S * e * nwin * dl, S * (k + p) * nwin * dl
    hm = _HostMem("pageable" if kind == "two-devices" else kind, inp.size + S * e * n + nod + nex + 4 * S + 4 * GUARD + 64)
    try:
        h_in, h_out, h_od, h_ex, h_m = _carve(hm.mem, [inp.size, S * e * n + GUARD, nod + GUARD, nex, 4 * S + GUARD + 8])
        h_m = h_m[(-h_m.ctypes.data) % 4:][:4 * S + GUARD].view(np.int32)
        h_in[:] = inp.reshape(-1)
        h_ex[:] = stored.reshape(-1)
        dec = rc.RawErasureDecoder(rc.ECReplicationConfig(k, p, codec))
        case = (codec, k, p, erased, kind, name)
        for ex in (h_ex, None):
            h_out[:] = 0x11
            h_od[:] = 0xA5
            h_m[:] = 0x5A5A5A5A
            dec.reconstruct_digest_host_batch(h_in, (k + p) * n, n, present, erased, h_out, e * n, n, S, n, typ, bpc, h_od,
                                              h_expected=ex, h_mismatch=h_m, stripes_per_chunk=2)
            assert (h_out[S * e * n:] == 0x11).all() and (h_od[nod:] == 0xA5).all() and (h_m[S:] == 0x5A5A5A5A).all()
            out, od = h_out[:S * e * n].reshape(S, e, n), h_od[:nod].reshape(S, e, nwin, dl)
            if ex is None:
                assert h_m[:S].tolist() == [-1] * S, case
                for s in (0, 2, 3, 4):
                    assert (out[s] == units[s, erased]).all() and (od[s] == dig[s, erased]).all(), (case, s)
            else:
                _rec_check(out, od, h_m[:S], S, units, dig, erased, bpc, name, want_m, case)
        del h_in, h_out, h_od, h_ex, h_m, out, od
    finally:
        hm.close()


# ---- stripe queue -----------------------------------------------------------------------------------------------------

def _cells(rng, k, n, pinned, keep, fill=None):
    out = []
    for _ in range(k):
        if pinned:
            pb = host_alloc(n)
            keep.append(pb)
            a = pb.array
        else:
            a = np.zeros(n, np.uint8)
        a[:] = rng.integers(0, 256, n, dtype=np.uint8) if fill is None else fill
        out.append(a)
    return out


def _queue_check(codec, k, p, name, dl, bpc, jobs):
    for t, d, par, digs, n in jobs:
        ref = _coded(codec, k, p, d)
        rows, nwin = len(ref), -(-n // bpc)
        for r in range(p):
            assert (par[r] == (ref[r] if r < rows else 0)).all(), (t, r)
        nd = (k + rows) * nwin * dl
        want = np.stack([_digests(name, u, bpc) for u in list(d) + ref])
        assert (digs[:nd].reshape(k + rows, nwin, dl) == want).all(), (t, n)
        assert (digs[nd:] == 0xA5).all(), (t, "guard")


@algos
@pytest.mark.parametrize("codec,k,p", [("rs", 6, 3), ("xor", 3, 2)])
def test_queue_digests_match_hashlib_and_oracle(codec, k, p, typ, name, dl):
    n, bpc, S = 65536, 16384, 4
    rows = 1 if codec == "xor" else p
    rng = np.random.default_rng([k, p, typ])
    enc = rc.RawErasureEncoder(rc.ECReplicationConfig(k, p, codec))
    keep, jobs = [], []
    with StripeQueue(enc, n, S, typ, bpc, big_endian=True) as q:
        for s in range(11):  # two full batches + a partial one, pinned and pageable buffers mixed
            pinned = s % 3 == 1
            d = _cells(rng, k, n, pinned, keep)
            par = _cells(rng, p, n, pinned and s % 2 == 1, keep, fill=0xA5)
            digs = np.full((k + rows) * (n // bpc) * dl + GUARD, 0xA5, np.uint8)
            jobs.append((q.submit(d, par, digests=digs), d, par, digs, n))
        q.wait(jobs[-1][0])
    _queue_check(codec, k, p, name, dl, bpc, jobs)
    for pb in keep:
        pb.free()


@algos
def test_queue_digests_mixed_lengths(typ, name, dl):
    k, p, cell, bpc = 6, 3, 1 << 16, 4096
    rng = np.random.default_rng([typ, 9])
    enc = rc.RawErasureEncoder(rc.ECReplicationConfig(k, p))
    q = StripeQueue(enc, cell, 8, typ, bpc)
    jobs = []
    for n in [cell, cell, 1000, 4096 + 16, cell, 17, cell]:
        d = _cells(rng, k, n, False, None)
        par = [np.zeros(n, np.uint8) for _ in range(p)]
        digs = np.full((k + p) * (-(-n // bpc)) * dl + GUARD, 0xA5, np.uint8)
        jobs.append((q.submit(d, par, digests=digs), d, par, digs, n))
    q.wait(jobs[3][0])
    _queue_check("rs", k, p, name, dl, bpc, jobs[:4])
    q.flush()
    q.wait(jobs[-1][0])
    _queue_check("rs", k, p, name, dl, bpc, jobs)
    q.close()


def test_queue_cross_errors_name_the_other_call():
    k, p, n = 3, 2, 512
    enc = rc.RawErasureEncoder(rc.ECReplicationConfig(k, p))
    d = [np.zeros(n, np.uint8) for _ in range(k)]
    par = [np.zeros(n, np.uint8) for _ in range(p)]
    with StripeQueue(enc, n, 2, ChecksumType.SHA256, 128) as q:
        with pytest.raises(Exception, match="ozec_stripe_queue_submit_digests"):
            q.submit(d, par, crcs=np.zeros(5 * 4, np.uint32))
    for ctype in (ChecksumType.CRC32C, ChecksumType.NONE):
        with StripeQueue(enc, n, 2, ctype, 128) as q:
            with pytest.raises(Exception, match="ozec_stripe_queue_submit"):
                q.submit(d, par, digests=np.zeros(5 * 4 * 32, np.uint8))
            assert "submit_digests" not in L.last_error()


# ---- argument errors that need a coder, and the counters ---------------------------------------------------------------

@algos
def test_argument_errors_with_a_coder(typ, name, dl):
    lib = L.lib()
    k, p, S, n, bpc = 3, 2, 2, 64, 16
    conf = rc.ECReplicationConfig(k, p)
    enc, dec = rc.RawErasureEncoder(conf), rc.RawErasureDecoder(conf)
    d_in = to_dev(np.zeros(S * (k + p) * n, np.uint8))
    d_out = to_dev(np.full(S * p * n, 0x11, np.uint8))
    d_dig = to_dev(np.full(S * (k + p) * 4 * dl, 0xA5, np.uint8))
    d_mis = to_dev(np.full(S, 0x5A5A5A5A, np.int32))
    i, o, g, m = d_in.data_ptr(), d_out.data_ptr(), d_dig.data_ptr(), d_mis.data_ptr()
    pres, er = L.int_array([1, 2, 3]), L.int_array([0])
    h_in, h_out, h_dig = np.zeros(S * (k + p) * n, np.uint8), np.zeros(S * p * n, np.uint8), np.zeros(4096, np.uint8)
    hi, ho, hg = h_in.ctypes.data, h_out.ctypes.data, h_dig.ctypes.data
    h_mis = np.full(S, 0x5A5A5A5A, np.int32)

    def enc_dev(c, a=i, b=o, c_=g, n_=n, s_=S):
        return lib.ozec_encode_digest_batch(c, a, k * n, n, b, p * n, n, s_, n_, typ, bpc, c_, None)

    def enc_host(c, a=hi, b=ho, c_=hg, n_=n, s_=S):
        return lib.ozec_encode_digest_host_batch(c, a, k * n, n, b, p * n, n, s_, n_, typ, bpc, c_, 0)

    def rec_dev(c, a=i, b=o, c_=g, ex=None, mm=m, n_=n, s_=S, bpc_=bpc):
        return lib.ozec_reconstruct_digest_batch(c, a, (k + p) * n, n, pres, 3, er, 1, b, n, n, s_, n_, typ, bpc_, ex, c_,
                                                 mm, None)

    def rec_host(c, a=hi, b=ho, c_=hg, ex=None, mm=h_mis.ctypes.data, n_=n, s_=S):
        return lib.ozec_reconstruct_digest_host_batch(c, a, (k + p) * n, n, pres, 3, er, 1, b, n, n, s_, n_, typ, bpc, ex,
                                                      c_, mm, 0)
    E, D = enc._handle, dec._handle
    for f in (enc_dev, enc_host):
        assert f(D) == L.OZEC_EINVAL and L.last_error() == "not an encoder"
        for kw in ({"a": None}, {"b": None}, {"c_": None}):
            assert f(E, **kw) == L.OZEC_EINVAL and "null" in L.last_error(), (f.__name__, kw)
        assert f(E, n_=0) == L.OZEC_OK and f(E, s_=0) == L.OZEC_OK
    for f in (rec_dev, rec_host):
        assert f(E) == L.OZEC_EINVAL and L.last_error() == "not a decoder"
        for kw in ({"a": None}, {"b": None}, {"c_": None}):
            assert f(D, **kw) == L.OZEC_EINVAL and "null" in L.last_error(), (f.__name__, kw)
        assert f(D, s_=0) == L.OZEC_OK
    assert rec_dev(D, ex=g, mm=None) == L.OZEC_EINVAL and "mismatch buffer" in L.last_error()
    # (k + p) * windows must fit the int32 mismatch report: refused before anything is launched
    assert rec_dev(D, n_=(1 << 31) // (k + p) + 1, bpc_=1) == L.OZEC_EINVAL and "int32" in L.last_error()
    torch.cuda.synchronize()
    assert (to_host(d_out) == 0x11).all() and (to_host(d_dig) == 0xA5).all() and (to_host(d_mis) == 0x5A5A5A5A).all()
    # len == 0: nothing written but the mismatch entries, which read -1
    assert rec_dev(D, n_=0) == L.OZEC_OK and rec_host(D, n_=0) == L.OZEC_OK
    assert (to_host(d_mis) == -1).all() and (h_mis == -1).all()
    assert (to_host(d_out) == 0x11).all() and (to_host(d_dig) == 0xA5).all()
    enc.release()
    dec.release()
    for f, c in ((enc_dev, E), (enc_host, E), (rec_dev, D), (rec_host, D)):
        assert f(c) == L.OZEC_ECLOSED and "closed" in L.last_error(), f.__name__


def test_counters_count_the_digest_calls():
    k, p, S, n, bpc, typ, dl = 3, 2, 2, 457, 100, 5, 16
    data, coded, units, dig = _reference("rs", k, p, S, n, bpc, 5)
    nwin = -(-n // bpc)
    conf = rc.ECReplicationConfig(k, p)
    enc, dec = rc.RawErasureEncoder(conf), rc.RawErasureDecoder(conf)
    before = L.stats()
    d_out = to_dev(np.zeros(S * p * n, np.uint8))
    d_dig = to_dev(np.zeros(S * (k + p) * nwin * dl, np.uint8))
    enc.encode_digest_batch(to_dev(data), k * n, n, d_out, p * n, n, S, n, typ, bpc, d_dig)
    d_o = to_dev(np.zeros(S * n, np.uint8))
    d_od = to_dev(np.zeros(S * nwin * dl, np.uint8))
    dec.reconstruct_digest_batch(to_dev(units), (k + p) * n, n, [1, 2, 3], [0], d_o, n, n, S, n, typ, bpc, d_od)
    torch.cuda.synchronize()
    h_out, h_dig = np.zeros(S * p * n, np.uint8), np.zeros(S * (k + p) * nwin * dl, np.uint8)
    enc.encode_digest_host_batch(np.ascontiguousarray(data), k * n, n, h_out, p * n, n, S, n, typ, bpc, h_dig)
    h_o, h_od = np.zeros(S * n, np.uint8), np.zeros(S * nwin * dl, np.uint8)
    dec.reconstruct_digest_host_batch(np.ascontiguousarray(units), (k + p) * n, n, [1, 2, 3], [0], h_o, n, n, S, n, typ,
                                      bpc, h_od)
    with StripeQueue(enc, n, 2, typ, bpc) as q:
        par = [np.zeros(n, np.uint8) for _ in range(p)]
        digs = np.zeros((k + p) * nwin * dl, np.uint8)
        q.wait(q.submit([np.ascontiguousarray(x) for x in data[0]], par, digests=digs))
    after = L.stats()
    for op, calls, nbytes in (("fused", 2, 2 * k * n * S), ("host_batch", 2, 2 * k * n * S)):
        assert after[op]["calls"] - before[op]["calls"] == calls, op
        assert after[op]["bytes"] - before[op]["bytes"] == nbytes, op
    assert after["queue"]["calls"] - before["queue"]["calls"] >= 2
    assert after["queue"]["bytes"] - before["queue"]["bytes"] == k * n
    assert (h_dig.reshape(S, k + p, nwin, dl) == dig["md5"]).all() and (h_o.reshape(S, n) == units[:, 0]).all()
    assert (to_host(d_od).reshape(S, nwin, dl) == dig["md5"][:, 0]).all() and (digs.reshape(k + p, nwin, dl) == dig["md5"][0]).all()
