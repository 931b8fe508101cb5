"""bench.py's host side, no GPU: the parallel DEM generation, --dump-outputs' files and the argument checks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_host_dem_in_child_processes_equals_synth_dem():
    """the bands made in child processes are the benchmark DEM itself, whole or one rank's rows"""
    from neilpy_amd.synth import synth_dem
    bench = bench_module()
    full = synth_dem(2304, seed=20240)
    assert np.array_equal(bench.host_dem(2304, np.float32, 0, 2304, 3), full)
    assert np.array_equal(bench.host_dem(2304, np.float32, 700, 2304, 2), full[700:])
    assert np.array_equal(bench.host_dem(2304, np.float64, 0, 2304, 2), synth_dem(2304, seed=20240, dtype=np.float64))


@pytest.mark.parametrize("n", [500, 3000])
def test_dump_outputs_files(tmp_path, n):
    """float32 / float64 files only, row and column sums over every cell, the whole mask or a seeded sample with its
    indices, under 64 MB; the same mask gives the same files"""
    import torch
    bench = bench_module()
    m = np.random.default_rng(4).random((n, n)) < 0.3
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.from_numpy(m), n, 0, n, 1, "cpu")
    files = sorted(os.listdir(tmp_path / "a"))
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) < 64 << 20
    assert np.array_equal(got["mask_row_sums"], m.sum(1)) and np.array_equal(got["mask_col_sums"], m.sum(0))
    if n * n <= bench.DUMP_FULL_CELLS:
        assert np.array_equal(got["mask"], m.astype(np.float32))
    else:
        idx = got["mask_sample_index"].astype(np.int64)
        assert len(idx) > bench.DUMP_SAMPLE // 2 and np.all(np.diff(idx) > 0)
        assert np.array_equal(got["mask_sample"], m.reshape(-1)[idx].astype(np.float32))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr and not r.stdout.strip()
