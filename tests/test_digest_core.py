"""CPU test of ozone_amd/csrc/digest_core.hpp, the SHA-256 / MD5 block functions and final-block padding the digest
kernels share with the host: tests/native/digest_core_main.cpp includes the header, is compiled with a plain g++ under
AddressSanitizer + UBSan and run as a program (no preload), and its output is compared with hashlib and with padding
built here from FIPS 180-4 section 5.1.1 / RFC 1321 section 3.1-3.2.  The padding cases reach the high word of the bit
length (totals of 2^29 and above), which no GPU test of a few seconds can."""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "digest_core_main.cpp")
LENGTHS = [1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 1000]
TOTALS = [1 << 29, (1 << 29) + 3, (1 << 32) + 5, (1 << 32) + 61]


def pattern(n):
    return bytes((i * 131 + (i >> 8) * 29 + 7) & 0xFF for i in range(n))


def spec_padding(algo, total):
    """The padded end of a message of `total` bytes whose last total % 64 bytes are tail byte j = (j * 37 + 11) & 0xff:
    0x80, zeros up to 56 mod 64, then the bit length in 8 bytes (SHA-256 big-endian, MD5 little-endian)."""
    r = total % 64
    tail = bytes((j * 37 + 11) & 0xFF for j in range(r))
    zeros = (55 - r) % 64
    bits = (total * 8) % (1 << 64)
    return tail + b"\x80" + bytes(zeros) + bits.to_bytes(8, "big" if algo == "sha256" else "little")


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("digest_core") / "digest_core_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-o", exe, SRC], check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, timeout=120, text=True).stdout
    return [line.split() for line in out.splitlines()]


def test_known_answers(records):
    abc = {r[1]: r[2] for r in records if r[0] == "abc"}
    assert abc["sha256"] == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    assert abc["md5"] == "900150983cd24fb0d6963f7d28e17f72"


@pytest.mark.parametrize("algo", ["sha256", "md5"])
def test_digests_match_hashlib(records, algo):
    got = {int(r[2]): r[3] for r in records if r[0] == "digest" and r[1] == algo}
    assert sorted(got) == LENGTHS
    for n in LENGTHS:
        assert got[n] == hashlib.new(algo, pattern(n)).hexdigest(), (algo, n)


@pytest.mark.parametrize("algo", ["sha256", "md5"])
def test_final_blocks_match_the_specification(records, algo):
    got = {int(r[2]): (int(r[3]), r[4]) for r in records if r[0] == "pad" and r[1] == algo}
    assert sorted(got) == TOTALS
    for total in TOTALS:
        want = spec_padding(algo, total)
        assert len(want) % 64 == 0
        assert got[total] == (len(want) // 64, want.hex()), (algo, total)
    assert got[(1 << 32) + 61][0] == 2 and got[(1 << 32) + 5][0] == 1  # both block counts, high length word set
