"""The stripe digest kernels of the shipped libozec.so (digest.hip: digest_stripes<A> for SHA-256 and for MD5 windows
under 256 bytes, digest_stripes_coop<MD5>) -- CPU test on the gfx950 code object.

Resources (scripts/kernel_resources.py): no scratch, no VGPR spills, at most 160 KiB of LDS; the cooperative form is
not instantiated for SHA-256 under the new name either.

Block loops (scripts/digest_bench.py loop_mix): a stripe kernel's block loop issues as many VALU instructions per
64-byte block as the cell kernel of the same algorithm and form, i.e. the load scheduling digest_blocks describes
survived the new addressing, and the cell kernels' own counts are those of the commit before the stripe kernels were
added, read from its build: 1,404 (SHA-256, simple form, two blocks per iteration), 324 (MD5, cooperative form, one block
per iteration) and 328 (MD5, simple form, two blocks per iteration).  Every load of the new kernels is a global_load:
an address that went through LDS must not have become a generic pointer (flat_load counts on the LDS counter too)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ozone_amd", "lib", "libozec.so")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (new kernel, existing kernel, digest::Algo, loop reads LDS, blocks per iteration, VALU per block before this change)
LOOPS = [("digest_stripes", "digest_windows", 0, False, 2, 1404),
         ("digest_stripes", "digest_windows", 1, False, 2, 328),
         ("digest_stripes_coop", "digest_windows_coop", 1, True, 1, 324)]
IDS = ["sha256", "md5-short-windows", "md5"]


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "libozec.so not built"
    import kernel_resources
    return kernel_resources.kernels(SO)


@pytest.fixture(scope="module")
def disassembly():
    assert os.path.exists(SO), "libozec.so not built"
    import isa_scan
    return isa_scan.disassemble_shared_object(SO)


def _new(kernel, algo):
    return f"{len(kernel)}{kernel}ILi{algo}EEEvN"


@pytest.mark.parametrize("kernel,algo", [(r[0], r[2]) for r in LOOPS], ids=IDS)
def test_stripe_digest_kernels_no_scratch_no_spills(kernels, kernel, algo):
    found = [k for k in kernels if _new(kernel, algo) in k["name"]]
    assert len(found) == 1, (_new(kernel, algo), [k["name"] for k in found])
    k = found[0]
    assert k.get("private_segment_fixed_size") == 0, k
    assert k.get("vgpr_spill_count") == 0, k
    assert k.get("group_segment_fixed_size", 0) <= 160 * 1024, k


def test_cooperative_stripe_form_is_not_shipped_for_sha256(kernels):
    assert not [k["name"] for k in kernels if "digest_stripes_coopILi0E" in k["name"]]


def _valu(mix):
    return sum(v for k, v in mix.items() if k.startswith("v_"))


@pytest.mark.parametrize("new,old,algo,lds,blocks,parent", LOOPS, ids=IDS)
def test_block_loop_valu_count_matches_the_cell_kernel(disassembly, new, old, algo, lds, blocks, parent):
    from digest_bench import loop_mix
    mix_old = loop_mix(disassembly, f"{old}ILi{algo}ELb0E", lds)
    mix_new = loop_mix(disassembly, f"{new}ILi{algo}EE", lds)
    print(new, algo, "VALU per block:", _valu(mix_new) / blocks, "cell kernel:", _valu(mix_old) / blocks)
    assert _valu(mix_old) == parent * blocks, (old, algo, _valu(mix_old) / blocks)
    assert _valu(mix_new) == _valu(mix_old), (new, algo, _valu(mix_new) / blocks, _valu(mix_old) / blocks)
    # the loads inside the loop are the cell kernel's: as many, none through the flat path
    for op in ("global_load_dwordx4", "ds_read_b128"):
        assert mix_new.get(op, 0) == mix_old.get(op, 0), (op, mix_new.get(op), mix_old.get(op))


@pytest.mark.parametrize("kernel,algo", [(r[0], r[2]) for r in LOOPS], ids=IDS)
def test_stripe_digest_kernels_load_through_global_not_flat(disassembly, kernel, algo):
    ops, on = [], False
    for line in disassembly.split("\n"):
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            on = f"{kernel}ILi{algo}EE" in m.group(2)
            continue
        m = re.match(r"^\s+(\S+)", line)
        if on and m:
            ops.append(m.group(1))
    assert any(o.startswith("global_load") for o in ops), kernel
    assert not [o for o in ops if o.startswith("flat_") or o.startswith("scratch_")], kernel
