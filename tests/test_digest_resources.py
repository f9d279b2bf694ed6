"""The SHA-256 / MD5 window-digest kernels of the shipped libozec.so -- digest.hip digest_windows<A, VERIFY> for both
algorithms, and digest_windows_coop<MD5, VERIFY>, the form MD5 windows of 256 bytes and more take -- use no scratch
memory, spill no VGPRs and fit the CU's 160 KiB of LDS (CPU test: reads the gfx950 code objects' metadata notes,
scripts/kernel_resources.py).  The cooperative form lost its A/B for SHA-256 and is not instantiated for it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ozone_amd", "lib", "libozec.so")
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "libozec.so not built"
    import kernel_resources
    return kernel_resources.kernels(SO)


# (kernel, digest::Algo): kSha256 = 0, kMd5 = 1
@pytest.mark.parametrize("kernel,algo", [("digest_windows", 0), ("digest_windows", 1), ("digest_windows_coop", 1)],
                         ids=["sha256", "md5-short-windows", "md5"])
@pytest.mark.parametrize("verify", [0, 1], ids=["compute", "verify"])
def test_digest_kernels_no_scratch_no_spills(kernels, kernel, algo, verify):
    pat = f"{len(kernel)}{kernel}ILi{algo}ELb{verify}EEEvN"
    found = [k for k in kernels if pat in k["name"]]
    assert len(found) == 1, (pat, [k["name"] for k in found])
    k = found[0]
    assert k.get("private_segment_fixed_size") == 0, k
    assert k.get("vgpr_spill_count") == 0, k
    assert k.get("group_segment_fixed_size", 0) <= 160 * 1024, k


def test_rejected_cooperative_form_is_not_shipped_for_sha256(kernels):
    assert not [k["name"] for k in kernels if "digest_windows_coopILi0E" in k["name"]]
