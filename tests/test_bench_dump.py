"""bench.py's plain / --full switch and the sampling of --dump-outputs (host arrays, CPU only): a plain run asks for
nothing but its timed steps, and the dumped arrays are exact float copies, whole when small, else a fixed sample that is
the same in every run and does not depend on the array's strides."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

EXTRAS = ("no_cpu", "no_e2e", "no_pmc", "no_legs", "no_inproc", "no_jni")


def test_plain_run_measures_the_headline_only():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs is None
    assert all(getattr(a, k) for k in EXTRAS)
    f = bench.parse(["--full"])
    assert f.full and not any(getattr(f, k) for k in EXTRAS)
    f = bench.parse(["--full", "--no-pmc"])
    assert f.no_pmc and not f.no_legs
    # the rocprofv3 children of a --full run are plain runs of one workload
    c = bench.parse(bench._child_base(f, "legs")[2:])
    assert c.workload == "legs" and not c.full and all(getattr(c, k) for k in EXTRAS)
    with pytest.raises(SystemExit):
        bench.parse(["--workload", "jni", "--dump-outputs", "x"])


def test_small_outputs_are_dumped_whole_and_exact():
    u8 = np.arange(3 * 5 * 7, dtype=np.uint8).reshape(3, 5, 7)
    got = bench._dump_array(u8[:, 2:], 1 << 20)
    assert got.dtype == np.float32 and got.shape == (3, 3, 7) and (got == u8[:, 2:]).all()
    crc = np.array([0, 1, -1, -(1 << 31), (1 << 31) - 1], dtype=np.int32)
    got = bench._dump_array(crc, 1 << 20)
    assert got.dtype == np.float64 and (got.astype(np.int64) == crc).all()
    got = bench._dump_array(crc.view(np.uint32), 1 << 20)
    assert got.dtype == np.float64 and (got.astype(np.uint64) == crc.view(np.uint32)).all()


def test_large_outputs_are_a_fixed_sample_in_runs():
    S, U, n, cap = 37, 9, 4099, 16 * bench.DUMP_RUN
    whole = np.random.default_rng(5).integers(0, 256, (S, U, n), dtype=np.uint8)
    par = whole[:, 6:]  # the parity units of a stripe-major batch: a strided view, as the device tensor is
    got = bench._dump_array(par, cap)
    assert got.dtype == np.float32 and got.shape == (cap,)
    assert (got == bench._dump_array(par, cap)).all()  # same elements every time
    assert (got == bench._dump_array(np.ascontiguousarray(par), cap)).all()  # whatever the strides
    flat = par.reshape(-1)
    span = flat.size // 16
    for r in range(16):  # one run of consecutive elements from each of the 16 equal spans
        run = got[r * bench.DUMP_RUN:(r + 1) * bench.DUMP_RUN].astype(np.uint8)
        windows = np.lib.stride_tricks.sliding_window_view(flat[r * span:(r + 1) * span], bench.DUMP_RUN)
        assert (windows == run).all(axis=1).any()


def test_dump_outputs_writes_one_file_per_output_within_the_budget(tmp_path):
    outs = {"parity": np.zeros((64, 3, 1 << 18), np.uint8), "crc": np.ones((64, 9, 16), np.int32)}
    bench.dump_outputs(outs, str(tmp_path / "d"), 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == ["crc.npy", "parity.npy"]
    p, c = np.load(tmp_path / "d" / "parity.npy"), np.load(tmp_path / "d" / "crc.npy")
    assert p.dtype == np.float32 and c.dtype == np.float64 and c.shape == (64, 9, 16) and (c == 1).all()
    assert p.nbytes + c.nbytes <= bench.DUMP_BYTES <= 64_000_000 and p.size == bench.DUMP_BYTES // 2 // 4
    bench.dump_outputs({"crc": outs["crc"]}, str(tmp_path / "e"), 1, 2)
    assert os.listdir(tmp_path / "e") == ["crc.rank1.npy"]
