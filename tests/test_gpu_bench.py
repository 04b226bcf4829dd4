"""bench.py's plain run and its --dump-outputs files: the headline fields, --steps honoured when the unsorted copies are refilled
between rounds, the dumped sample and chunk sums equal to the sorted input, the same files from two runs, and --full still
carrying the figures it moved behind it."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import reference_sorted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3_000_003   # three chunk sums, the last one partial


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run_main(bench, monkeypatch, capsys, argv):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["u32", "u64", "f32"])
def test_plain_run_dumps_the_sorted_keys(gpu, tmp_path, monkeypatch, capsys, dt):
    import torch
    bench = _load_bench()
    monkeypatch.setattr(bench, "pool_size", lambda torch, src, want: min(want, 2))   # 6 steps in rounds of 2 copies
    line = _run_main(bench, monkeypatch, capsys, ["--keys", str(N), "--steps", "5", "--warmup", "1", "--dtype", dt,
                                                  "--dump-outputs", str(tmp_path)])
    assert line["metric"] == f"radix_sort_throughput_1B_uniform_{dt}" and line["unit"] == "Gkeys/s"
    assert line["higher_is_better"] is True and line["dtype"] == dt and line["steps"] == 5 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3) / 1e9, rel=1e-2)
    for moved in ("roofline", "kernels", "copy_ceiling", "configs", "end_to_end", "cpu_baseline"):
        assert moved not in line

    files = {f: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(files) == {"sorted_keys_sample.npy", "sample_positions.npy", "sorted_keys_chunk_sums.npy"}
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())

    _v, npdt, kb, _lv, seed = bench.DTYPES[dt]
    src = bench.gen_keys(torch, N, dt, seed).cpu().numpy().view(npdt)
    u = reference_sorted(src).view(f"u{kb}")
    pos = files["sample_positions.npy"].astype(np.int64)
    assert len(pos) == min(N, bench.DUMP_SAMPLE) and np.all(np.diff(pos) >= 0)
    sample = files["sorted_keys_sample.npy"]
    lo32 = np.uint64(0xFFFFFFFF)
    if dt == "f32":
        assert sample.dtype == np.float32 and np.array_equal(sample.view(np.uint32), u[pos])
    elif dt == "u32":
        assert np.array_equal(sample, u[pos].astype(np.float64))
    else:
        assert np.array_equal(sample, np.stack((u[pos] >> np.uint64(32), u[pos] & lo32), 1).astype(np.float64))
    words = u.astype(np.uint64)[:, None] if kb == 4 else np.stack((u >> np.uint64(32), u & lo32), 1)
    c = bench.DUMP_CHUNK
    want = np.stack([words[s:s + c].sum(0) for s in range(0, N, c)]).astype(np.float64)
    assert np.array_equal(files["sorted_keys_chunk_sums.npy"], want[:, 0] if kb == 4 else want)


@pytest.mark.gpu
def test_dumps_of_two_runs_are_identical(gpu, tmp_path):
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--keys", "2000000", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 3
    for f in names:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f


@pytest.mark.gpu
def test_full_run_keeps_the_other_figures(gpu, monkeypatch, capsys):
    bench = _load_bench()
    line = _run_main(bench, monkeypatch, capsys, ["--keys", str(N), "--steps", "3", "--warmup", "1", "--full", "--no-big"])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert "roofline" in line and line["kernels"]
    assert {"copy", "read", "write"} <= set(line["copy_ceiling"])
    assert line["end_to_end"]["ms"] > 0
    assert line["cpu_baseline"]["bit_identical_to_device_output"] is True
