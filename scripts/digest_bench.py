"""SHA256 / MD5 window digests on the GPU: rates, the VALU ceiling, HBM traffic and the host-path crossover.

One process, warm-up then timed repetitions, median and spread per row, one JSON:

  python scripts/digest_bench.py [--out profiles/digest/digest_bench.json] [--reps 9]

  device    ozec_digest_windows_batch / ozec_digest_verify_batch on 3,072 cells of 1 MiB, bpc = 16 KiB and 1 MiB, device
            events around each launch, GB/s of data hashed
  valu      VALU instructions per 64-byte block counted in the hot loop of the shipped code object, the issue rate of
            those instructions from scripts/valu_rate (built with hipcc when the binary is absent), the ceiling that
            follows and the fraction reached
  host      ozec_digest_windows on 1 / 4 / 16 / 64 MiB pinned and pageable buffers against hashlib on 1 and 16 threads,
            and the size from which the GPU path is faster than each

HBM traffic comes from a counters-only profiler pass of its own (no tracing beside the counters), whose CSV is merged
into the JSON afterwards:

  rocprofv3 --pmc FETCH_SIZE -d DIR -o run --output-format csv -- python scripts/digest_bench.py --pmc-kernels
  python scripts/digest_bench.py --merge-pmc DIR --out profiles/digest/digest_bench.json

The stripe paths (ozec_encode_digest_batch and its host form, DESIGN 2.6 "stripes" and 3) have a run of their own:

  python scripts/digest_bench.py --stripes [--out profiles/digest/stripe_digest_bench.json] [--reps 9]

  device    rs-6-3, 1 MiB cells, 341 stripes, bpc 16 KiB and 1 MiB: ozec_encode_digest_batch against ozec_encode_batch
            followed by ozec_digest_windows_batch over the uniform [S][k+p] layout, alternated in one loop
  small     one queue batch (64 stripes) and one host chunk (32 stripes): the one-launch call, the same work with two
            digest launches (data cells, parity cells), and the floor -- one lane's serial walk over one window
  host      ozec_encode_digest_host_batch (SHA256, MD5) against ozec_encode_crc_host_batch (CRC32C) on one pinned batch,
            alternated, bpc 16 KiB and 1 MiB

There is no fallback: without a GPU the device, valu-rate and host sections fail.
"""
import argparse
import concurrent.futures
import csv
import glob
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CELLS, CELL = 3072, 1 << 20
ALGOS = [("sha256", 4, 32, 0), ("md5", 5, 16, 1)]  # name, ChecksumType, digest length, digest::Algo
SIMDS = 256 * 4
FORM = {"sha256": "simple", "md5": "coop"}  # the fetch form each algorithm ships with (digest.hip kCoop)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


# ---- VALU instructions per block, from the shipped code object ------------------------------------------------------

def loop_mix(text, kernel_pat, want_lds):
    """Instruction mix of a kernel's block loop in an llvm-objdump disassembly: the innermost loop (a backward branch
    with no other inside it) with the most instructions among those that do (cooperative form: the loop over the four
    blocks of a step) or do not (simple form: the two-block loop) read LDS."""
    body, on = [], False
    for line in text.split("\n"):
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            on = kernel_pat in m.group(2)
            continue
        m = re.match(r"^\s+(\S+)(.*?)//\s*([0-9A-F]+):", line)
        if on and m:
            body.append((int(m.group(3), 16), m.group(1), m.group(2).strip()))
    assert body, kernel_pat
    loops = []
    for addr, op, args in body:
        if op.startswith("s_cbranch") or op == "s_branch":
            off = int(args.split()[0])
            if off >= 32768:
                loops.append((addr + 4 + (off - 65536) * 4, addr))
    inner = [(lo, hi) for lo, hi in loops if not any((a, b) != (lo, hi) and lo <= a and b <= hi for a, b in loops)]
    best = None
    for lo, hi in inner:
        ops = [op for a, op, _ in body if lo <= a <= hi]
        if any(o.startswith("ds_read") for o in ops) == want_lds and (best is None or len(ops) > len(best)):
            best = ops
    assert best, (kernel_pat, want_lds)
    return Counter(best)


def valu_counts():
    import isa_scan
    text = isa_scan.disassemble_shared_object(os.path.join(ROOT, "ozone_amd", "lib", "libozec.so"))
    out = {}
    for name, _, _, algo in ALGOS:
        # the loop the 16 KiB rows spend their time in: SHA-256 the simple form's two-block loop (digest_windows<0, false>,
        # mangled), MD5 the cooperative form's loop over the four blocks of a step, one block per iteration
        if name == "md5":
            mix, blocks = loop_mix(text, f"digest_windows_coopILi{algo}ELb0E", True), 1
        else:
            mix, blocks = loop_mix(text, f"digest_windowsILi{algo}ELb0E", False), 2
        valu = sum(v for k, v in mix.items() if k.startswith("v_"))
        out[name] = {"loop_instructions": sum(mix.values()), "blocks_per_iteration": blocks,
                     "valu_per_block": valu / blocks, "valu_per_byte": valu / blocks / 64,
                     "mix_per_block": {k: v / blocks for k, v in mix.most_common(12)}}
    return out


def valu_rate():
    """G wave-instructions per second per SIMD of the digest kernels' instruction kinds, at 2 and 4 waves per SIMD"""
    exe = os.path.join(ROOT, "scripts", "valu_rate")
    if not os.path.exists(exe):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", exe + ".hip", "-o", exe], check=True,
                       timeout=600)
    txt = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout
    rates = {}
    for line in txt.splitlines():
        m = re.match(r"^(\S+)\s+W=(\d+)\s.*clk ([\d.]+) GHz.*-> ([\d.]+) G instr/s/SIMD", line)
        if m and m.group(1) in ("v_bitop3_b32", "v_alignbit_b32", "v_add_u32", "v_perm_b32", "v_xad_u32"):
            rates.setdefault(m.group(1), {})[f"W{m.group(2)}"] = {"G_instr_per_s_per_SIMD": float(m.group(4)),
                                                                 "clock_GHz": float(m.group(3))}
    assert rates, txt[-2000:]
    return rates


# ---- device-resident rates ---------------------------------------------------------------------------------------------

def device_rows(reps, warmup):
    import torch
    from devcopy import to_host
    from ozone_amd import _lib as L
    from ozone_amd import checksum as ck
    assert torch.cuda.is_available(), "digest_bench needs a GPU"
    lib = L.lib()
    data = torch.empty(CELLS * CELL, dtype=torch.uint8, device="cuda:0")
    assert lib.ozec_fill_splitmix64_cells(data.data_ptr(), CELL, CELLS, CELL, 0xD16E57, 0, None) == 0
    torch.cuda.synchronize()
    rows = []
    for name, typ, dl, _ in ALGOS:
        for bpc in (16384, 1 << 20):
            nwin = CELL // bpc
            out = torch.zeros(CELLS * nwin * dl, dtype=torch.uint8, device="cuda:0")
            mis = torch.zeros(CELLS, dtype=torch.int32, device="cuda:0")
            calls = {"digest_windows_batch": lambda: ck.digest_windows_batch(typ, data, CELL, CELLS, CELL, bpc, out),
                     "digest_verify_batch": lambda: ck.digest_verify_batch(typ, data, CELL, CELLS, CELL, bpc, out,
                                                                           mis)}
            for call, fn in calls.items():
                n = max(3, reps // 3) if bpc == 1 << 20 else reps  # one lane per cell: tens of ms per launch
                for _ in range(warmup):
                    fn()
                torch.cuda.synchronize()
                ms = []
                for _ in range(n):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                gbs = [CELLS * CELL / (t * 1e-3) / 1e9 for t in ms]
                row = {"algo": name, "call": call, "form": FORM[name], "bytes_per_checksum": bpc,
                       "cells": CELLS, "cell_bytes": CELL, "ms": spread(ms), "GBps": spread(gbs)}
                if call == "digest_verify_batch":  # the expected digests are the ones just computed
                    row["all_match"] = bool((to_host(mis) == -1).all())
                    assert row["all_match"]
                else:  # spot check against hashlib: first and last cell
                    h = to_host(out).reshape(CELLS, nwin, dl)
                    for c in (0, CELLS - 1):
                        cell = to_host(data[c * CELL:(c + 1) * CELL]).tobytes()
                        for w in (0, nwin - 1):
                            assert h[c, w].tobytes() == hashlib.new(name, cell[w * bpc:(w + 1) * bpc]).digest()
                rows.append(row)
                print(json.dumps(row), flush=True)
    del data
    torch.cuda.empty_cache()
    return rows


def pmc_kernels():
    """one launch of each kernel on the 3 GiB device shape (past the 256 MiB Infinity Cache), for a counters-only pass"""
    import torch
    from ozone_amd import _lib as L
    from ozone_amd import checksum as ck
    lib = L.lib()
    data = torch.empty(CELLS * CELL, dtype=torch.uint8, device="cuda:0")
    assert lib.ozec_fill_splitmix64_cells(data.data_ptr(), CELL, CELLS, CELL, 0xD16E57, 0, None) == 0
    bpc = 16384
    for name, typ, dl, _ in ALGOS:
        out = torch.zeros(CELLS * (CELL // bpc) * dl, dtype=torch.uint8, device="cuda:0")
        for _ in range(2):
            ck.digest_windows_batch(typ, data, CELL, CELLS, CELL, bpc, out)
        torch.cuda.synchronize()
    print("pmc kernels done")


def merge_pmc(pmc_dir, out_path):
    paths = glob.glob(os.path.join(pmc_dir, "**", "*counter_collection.csv"), recursive=True)
    assert paths, pmc_dir
    per = {}
    for p in paths:
        for r in csv.DictReader(open(p)):
            if (("digest_windows" in r["Kernel_Name"] or "digest_stripes" in r["Kernel_Name"])
                    and r["Counter_Name"] == "FETCH_SIZE"):
                per.setdefault(r["Kernel_Name"], []).append(float(r["Counter_Value"]))
    res = json.load(open(out_path))
    # --pmc-kernels: 3,072 cells; --stripes-pmc-kernels: 341 stripes of 9 cells
    alg = 341 * 9 * CELL if any("digest_stripes" in k for k in per) else CELLS * CELL
    res["hbm_traffic"] = {
        "source": "rocprofv3 --pmc FETCH_SIZE, counters only, one pass; bytes = 2 * FETCH_SIZE * 1024 on gfx950",
        "shape": f"{CELLS} cells of {CELL} bytes, bpc 16384", "algorithmic_bytes": alg,
        "kernels": {k: {"FETCH_SIZE_KiB": v, "hbm_bytes": [2 * x * 1024 for x in v],
                        "hbm_over_algorithmic": [2 * x * 1024 / alg for x in v]} for k, v in sorted(per.items())}}
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res["hbm_traffic"], indent=1))


# ---- host path -----------------------------------------------------------------------------------------------------------

def host_rows(reps):
    import numpy as np
    from ozone_amd import _lib as L
    from ozone_amd.stripe_queue import host_alloc
    lib = L.lib()
    bpc = 16384
    rows = []
    pool16 = concurrent.futures.ThreadPoolExecutor(16)

    def hashlib_windows(name, buf, threads):
        mv = memoryview(buf)
        offs = range(0, len(mv), bpc)
        one = lambda o: hashlib.new(name, mv[o:o + bpc]).digest()  # noqa: E731  (hashlib drops the GIL above 2 KiB)
        if threads == 1:
            return [one(o) for o in offs]
        span = (len(offs) + threads - 1) // threads
        parts = [offs[i:i + span] for i in range(0, len(offs), span)]
        return [d for part in pool16.map(lambda p: [one(o) for o in p], parts) for d in part]

    for mib in (1, 4, 16, 64):
        n = mib << 20
        rng = np.random.default_rng(mib)
        src = rng.integers(0, 256, n, dtype=np.uint8)
        for name, typ, dl, _ in ALGOS:
            nout = n // bpc * dl
            want = b"".join(hashlib_windows(name, src, 1))
            row = {"algo": name, "bytes": n, "bytes_per_checksum": bpc}
            for threads in (1, 16):
                ts = []
                for _ in range(max(3, reps // 2)):
                    t0 = time.perf_counter()
                    hashlib_windows(name, src, threads)
                    ts.append((time.perf_counter() - t0) * 1e3)
                row[f"hashlib_{threads}t_ms"] = spread(ts)
            pool = host_alloc(n + nout + 4096)
            pin_src = pool.array[:n]
            pin_src[:] = src
            pin_out = pool.array[n + 256:n + 256 + nout]
            page_out = np.zeros(nout, np.uint8)
            for kind, s, o in (("pageable", src, page_out), ("pinned", pin_src, pin_out)):
                ts = []
                for i in range(2 + reps):
                    t0 = time.perf_counter()
                    rc = lib.ozec_digest_windows(typ, s.ctypes.data, n, bpc, o.ctypes.data)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert rc == 0, L.last_error()
                    if i >= 2:
                        ts.append(dt)
                assert o.tobytes() == want, (name, kind, mib)
                row[f"gpu_{kind}_ms"] = spread(ts)
                row[f"gpu_{kind}_GBps"] = n / (statistics.median(ts) * 1e-3) / 1e9
            del pin_src, pin_out
            pool.free()
            rows.append(row)
            print(json.dumps(row), flush=True)
    cross = {}
    for name, *_ in ALGOS:
        for kind in ("pageable", "pinned"):
            for threads in (1, 16):
                wins = [r["bytes"] for r in rows if r["algo"] == name and
                        r[f"gpu_{kind}_ms"]["median"] < r[f"hashlib_{threads}t_ms"]["median"]]
                loses = [r["bytes"] for r in rows if r["algo"] == name and r["bytes"] not in wins]
                # faster from a size on: every measured size at or above it wins
                frm = min((b for b in wins if all(x < b for x in loses)), default=None)
                cross[f"{name}_{kind}_vs_hashlib_{threads}t"] = frm
    return rows, cross


# ---- stripes: encode + digests in one call ---------------------------------------------------------------------------------

def _alternate(fns, reps, warmup, timer):
    """every function `warmup` times, then `reps` rounds in which each runs once, the order reversed every other round;
    {name: [ms]}"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in fns}
    order = list(fns)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):  # no version always runs behind the same other one
            ms[k].append(timer(fns[k]))
    return ms


def stripe_rows(reps, warmup):
    import numpy as np
    import torch
    from devcopy import to_host
    from ozone_amd import _lib as L
    from ozone_amd import checksum as ck
    from ozone_amd import rawcoder as rc
    from ozone_amd.stripe_queue import host_alloc
    assert torch.cuda.is_available(), "digest_bench needs a GPU"
    lib = L.lib()
    k, p, n = 6, 3, CELL
    enc = rc.RawErasureEncoder(rc.ECReplicationConfig(k, p))

    def ev(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    res = {"device_resident": [], "small_launches": [], "host": []}
    S = 341
    units = torch.empty(S * (k + p) * n, dtype=torch.uint8, device="cuda:0")
    assert lib.ozec_fill_splitmix64_cells(units.data_ptr(), n, S * (k + p), n, 0xD16E57, 0, None) == 0
    par = units[k * n:]
    torch.cuda.synchronize()
    for name, typ, dl, _ in ALGOS:
        for bpc in (16384, 1 << 20):
            nwin = n // bpc
            dig = torch.zeros(S * (k + p) * nwin * dl, dtype=torch.uint8, device="cuda:0")
            dig2 = torch.zeros_like(dig)

            def one(dig=dig, bpc=bpc, typ=typ):
                enc.encode_digest_batch(units, (k + p) * n, n, par, (k + p) * n, n, S, n, typ, bpc, dig)

            def two(dig2=dig2, bpc=bpc, typ=typ):
                enc.encode_batch(units, (k + p) * n, n, par, (k + p) * n, n, S, n)
                ck.digest_windows_batch(typ, units, n, S * (k + p), n, bpc, dig2)
            ms = _alternate({"encode_digest_batch": one, "encode_batch+digest_windows_batch": two},
                            max(3, reps // 3) if bpc == 1 << 20 else reps, warmup, ev)
            a, b = to_host(dig), to_host(dig2)
            assert (a == b).all()  # same layout [S][k+p][nwin][dl]; spot check against hashlib below
            u0 = to_host(units[:n]).tobytes()
            assert a[:dl].tobytes() == hashlib.new(name, u0[:bpc]).digest()
            row = {"algo": name, "bytes_per_checksum": bpc, "stripes": S, "cell_bytes": n, "schema": "rs-6-3",
                   "ms": {c: spread(v) for c, v in ms.items()},
                   "GBps_of_data": {c: S * k * n / (statistics.median(v) * 1e-3) / 1e9 for c, v in ms.items()}}
            res["device_resident"].append(row)
            print(json.dumps(row), flush=True)
            del dig, dig2
    # small launches, data and parity in two allocations as a queue batch / host chunk holds them
    for name, typ, dl, _ in ALGOS:
        bpc = 16384
        nwin = n // bpc
        one_win = torch.zeros(dl, dtype=torch.uint8, device="cuda:0")
        for Ss, what in ((64, "queue batch"), (32, "host chunk")):
            data = units[:Ss * k * n]
            parity = torch.empty(Ss * p * n, dtype=torch.uint8, device="cuda:0")
            dig = torch.zeros(Ss * (k + p) * nwin * dl, dtype=torch.uint8, device="cuda:0")
            dd = torch.zeros(Ss * k * nwin * dl, dtype=torch.uint8, device="cuda:0")
            dp = torch.zeros(Ss * p * nwin * dl, dtype=torch.uint8, device="cuda:0")
            fns = {
                "encode_digest_batch": lambda: enc.encode_digest_batch(data, k * n, n, parity, p * n, n, Ss, n, typ, bpc,
                                                                       dig),
                "encode_batch": lambda: enc.encode_batch(data, k * n, n, parity, p * n, n, Ss, n),
                "encode_batch+two_digest_launches": lambda: (
                    enc.encode_batch(data, k * n, n, parity, p * n, n, Ss, n),
                    ck.digest_windows_batch(typ, data, n, Ss * k, n, bpc, dd),
                    ck.digest_windows_batch(typ, parity, n, Ss * p, n, bpc, dp)),
                "one_lane_one_window": lambda: ck.digest_windows_batch(typ, data, n, 1, bpc, bpc, one_win),
            }
            ms = _alternate(fns, reps, warmup, ev)
            row = {"algo": name, "what": what, "stripes": Ss, "bytes_per_checksum": bpc, "lanes": Ss * (k + p) * nwin,
                   "ms": {c: spread(v) for c, v in ms.items()}}
            res["small_launches"].append(row)
            print(json.dumps(row), flush=True)
    del units, par
    torch.cuda.empty_cache()
    # from host memory: one pinned batch, CRC32C against the digests
    Sh = 128
    crc_bytes = Sh * (k + p) * (n // 16384) * 32
    pool = host_alloc(Sh * (k + p) * n + crc_bytes + 4096)
    h_in = pool.array[:Sh * k * n]
    h_in.reshape(-1, 1 << 20)[:] = np.random.default_rng(3).integers(0, 256, 1 << 20, dtype=np.uint8)
    h_out = pool.array[Sh * k * n:Sh * (k + p) * n]
    h_sum = pool.array[Sh * (k + p) * n + 256:Sh * (k + p) * n + 256 + crc_bytes]
    for bpc in (16384, 1 << 20):
        fns = {"crc32c": lambda: enc.encode_crc_host_batch(h_in, k * n, n, h_out, p * n, n, Sh, n, 3, bpc,
                                                           h_sum.ctypes.data)}
        for name, typ, dl, _ in ALGOS:
            fns[name] = lambda typ=typ: enc.encode_digest_host_batch(h_in, k * n, n, h_out, p * n, n, Sh, n, typ, bpc,
                                                                     h_sum)
        ms = _alternate(fns, max(3, reps // 2), 1, wall)
        row = {"bytes_per_checksum": bpc, "stripes": Sh, "cell_bytes": n, "schema": "rs-6-3", "buffers": "pinned",
               "stripes_per_chunk": 32, "ms": {c: spread(v) for c, v in ms.items()},
               "GBps_of_data": {c: Sh * k * n / (statistics.median(v) * 1e-3) / 1e9 for c, v in ms.items()}}
        res["host"].append(row)
        print(json.dumps(row), flush=True)
    del h_in, h_out, h_sum
    pool.free()
    return res


def stripe_pmc_kernels():
    """one encode_digest_batch per algorithm on the 341-stripe shape, for a counters-only pass (FETCH_SIZE of the stripe
    kernels against the cell kernels' 1.013-1.016 of the algorithmic bytes)"""
    import torch
    from ozone_amd import _lib as L
    from ozone_amd import rawcoder as rc
    lib = L.lib()
    k, p, n, S, bpc = 6, 3, CELL, 341, 16384
    units = torch.empty(S * (k + p) * n, dtype=torch.uint8, device="cuda:0")
    assert lib.ozec_fill_splitmix64_cells(units.data_ptr(), n, S * (k + p), n, 0xD16E57, 0, None) == 0
    enc = rc.RawErasureEncoder(rc.ECReplicationConfig(k, p))
    for name, typ, dl, _ in ALGOS:
        dig = torch.zeros(S * (k + p) * (n // bpc) * dl, dtype=torch.uint8, device="cuda:0")
        for _ in range(2):
            enc.encode_digest_batch(units, (k + p) * n, n, units[k * n:], (k + p) * n, n, S, n, typ, bpc, dig)
        torch.cuda.synchronize()
    print("pmc kernels done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "digest", "digest_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--pmc-kernels", action="store_true", help="only launch each kernel (for a rocprofv3 --pmc pass)")
    ap.add_argument("--merge-pmc", metavar="DIR", help="merge a --pmc pass's counter CSV into --out")
    ap.add_argument("--stripes", action="store_true", help="the stripe paths: encode + digests in one call")
    ap.add_argument("--stripes-pmc-kernels", action="store_true", help="only launch the stripe kernels (for --pmc)")
    a = ap.parse_args()
    if a.stripes_pmc_kernels:
        return stripe_pmc_kernels()
    if a.stripes:
        out = a.out if a.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "digest",
                                                                        "stripe_digest_bench.json")
        res = stripe_rows(a.reps, a.warmup)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)
        print("wrote", out)
        return
    if a.merge_pmc:
        return merge_pmc(a.merge_pmc, a.out)
    if a.pmc_kernels:
        return pmc_kernels()
    res = {"device_resident": device_rows(a.reps, a.warmup)}
    counts, rates = valu_counts(), valu_rate()
    res["valu"] = {"instructions": counts, "issue_rate": rates, "ceiling": {}}
    for name, *_ in ALGOS:
        mix = counts[name]["mix_per_block"]
        known = {k: rates[k]["W4"]["G_instr_per_s_per_SIMD"] for k in rates if "W4" in rates[k]}
        other = known.get("v_add_u32", min(known.values()))
        vpb = counts[name]["valu_per_block"]
        listed = sum(v for k, v in mix.items() if k.startswith("v_"))
        # seconds of issue per block per SIMD: each instruction kind at its own measured rate, the rest at v_add_u32's
        ns = sum(v / known.get(k.replace("_e32", "").replace("_e64", ""), other) for k, v in mix.items()
                 if k.startswith("v_")) + (vpb - listed) / other
        ceiling = SIMDS * 64 * 64 / ns  # a wave instruction serves 64 lanes = 64 blocks of 64 bytes; ns -> GB/s
        best = max(r["GBps"]["median"] for r in res["device_resident"]
                   if r["algo"] == name and r["call"] == "digest_windows_batch" and r["bytes_per_checksum"] == 16384)
        res["valu"]["ceiling"][name] = {
            "arithmetic": f"{SIMDS} SIMDs x 64 lanes x 64 B / {ns:.1f} ns of VALU issue per block",
            "issue_ns_per_block": ns, "ceiling_GBps": ceiling, "reached_GBps": best, "fraction": best / ceiling}
    print(json.dumps(res["valu"]["ceiling"], indent=1), flush=True)
    if not a.skip_host:
        res["host_path"], res["host_crossover_bytes"] = host_rows(a.reps)
        print(json.dumps(res["host_crossover_bytes"], indent=1), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
