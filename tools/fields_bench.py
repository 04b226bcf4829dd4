"""Timings of the described-key records route (rdst_key_field tables).  A development aid, not the benchmark.

    python tools/fields_bench.py [--rows 10000000] [--reps 5] [--out profiles/fields_bench.json]
    python tools/fields_bench.py --nowait [--rows 10000000] [--reps 5] [--out FILE]

On --rows records of 32 bytes:
  (a) rdst_hip_sort_records with one f32 field                      host entry, wall clock (the call blocks)
  (b) rdst_hip_sort_records_by_fields with the same single field    host entry, wall clock; (a) and (b) alternate
  (c) rdst_hip_sort_records_by_fields_device with (u16, i64), L=10  device entry, HIP events (it blocks: L > 8)
  (d) pack_fields_kernel alone (rdst_hip_pack_fields_device)        HIP events, for the keys of (b) and (c), next to
      rdst_hip_stream_copy over as many bytes as the kernel reads and writes, in the same run
Every case runs once untimed, then --reps times; every sort starts from a fresh copy of the same input (not timed).  The
yardstick for (b) is (a): the ratio of medians is printed next to the spread (max / min) that (a) shows against itself.

--nowait: case (c) alone, through rdst_hip_sort_records_by_fields_device and rdst_hip_sort_records_by_fields_device_nowait
in the same process, alternating; both medians and their ratio.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REC = 32


def _stats(ms):
    ms = sorted(ms)
    return {"ms": round(ms[len(ms) // 2], 3), "ms_all": [round(x, 3) for x in ms], "spread": round(ms[-1] / ms[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nowait", action="store_true", help="case (c) through the blocking and the nowait entry, alternating")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import rdst_amd
    from rdst_amd import _lib
    from rdst_amd.radix_sort import KeyField, _field_table
    assert torch.cuda.is_available(), "fields_bench needs a HIP device"
    torch.cuda.set_device(0)
    lib = _lib.load()
    n, reps = args.rows, args.reps
    dt = np.dtype({"names": ["score", "tenant", "ts", "rest"], "formats": ["<f4", "<u2", "<i8", "V12"], "offsets": [0, 4, 8, 16], "itemsize": REC})
    rng = np.random.default_rng(32)
    src = np.zeros(n, dtype=dt)
    src["score"] = rng.standard_normal(n).astype(np.float32)
    src["tenant"] = rng.integers(0, 1000, size=n)
    src["ts"] = rng.integers(-2**40, 2**40, size=n)
    one = [KeyField(0, 4, "float")]
    two = rdst_amd.key_fields_of(dt, ["tenant", "ts"])
    results = {}

    if args.nowait:
        dev_src = torch.from_numpy(src.view(np.uint8).reshape(n, REC)).cuda()
        dev = torch.empty_like(dev_src)
        table2, nf2 = _field_table(two)
        scratch = torch.empty(int(lib.rdst_hip_sort_records_by_fields_scratch_bytes(n, REC, table2, nf2)), dtype=torch.uint8, device="cuda")
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        entries = {"blocking": rdst_amd.sort_records_device_tensor, "nowait": rdst_amd.sort_records_device_nowait_tensor}
        ms, out = {k: [] for k in entries}, {}
        for rep in range(reps + 1):
            for name, sort in entries.items():
                dev.copy_(dev_src)
                torch.cuda.synchronize()
                start.record()
                sort(dev, two, scratch=scratch, check=False)
                stop.record()
                stop.synchronize()
                if rep:
                    ms[name].append(start.elapsed_time(stop))
                else:
                    out[name] = dev.clone()
        rdst_amd.device_status()
        assert torch.equal(out["blocking"], out["nowait"])
        # rows whose 8-byte prefix (tenant, the top six bytes of the mapped ts) equals another's: one is enough to raise the flag
        prefix = np.sort((src["tenant"].astype(np.uint64) << np.uint64(48)) | ((src["ts"].astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)) >> np.uint64(16)))
        same = prefix[1:] == prefix[:-1]
        tied = int(np.count_nonzero(np.concatenate(([False], same)) | np.concatenate((same, [False]))))
        ratio = round(_stats(ms["nowait"])["ms"] / _stats(ms["blocking"])["ms"], 3)
        results["c_device_u16_i64"] = {"blocking": _stats(ms["blocking"]), "nowait": _stats(ms["nowait"]), "key_bytes": 10, "rounds": 2,
                                       "rows_with_a_tied_prefix": tied, "nowait_over_blocking": ratio}
        if ratio > 1.5:                                    # the pair sorts' stage times, one more run each under rdst_hip_set_profiling
            for name, sort in entries.items():
                rdst_amd.set_profiling(True)
                dev.copy_(dev_src)
                torch.cuda.synchronize()
                sort(dev, two, scratch=scratch, check=False)
                torch.cuda.synchronize()
                runs = []
                for r in range(rdst_amd.profile_runs()):
                    got = rdst_amd.profile_run(r, 0)
                    by = {}
                    for stage, _level, t in (got["stages"] if got else ()):
                        by[stage] = round(by.get(stage, 0.0) + t, 3)
                    runs.append(by)
                rdst_amd.set_profiling(False)
                results["c_device_u16_i64"][name + "_pair_sort_stages_ms"] = runs
            rdst_amd.device_status()
        summary = {"tool": "tools/fields_bench.py --nowait", "device": torch.cuda.get_device_name(0), "rows": n, "record_bytes": REC, "reps": reps,
                   "results": results}
        print(json.dumps(summary))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(summary, f, indent=1)
        return

    # (a), (b): alternating, one warm-up each
    work = src.copy()
    ms = {"a": [], "b": []}
    sorted_by = {}
    for rep in range(reps + 1):
        for case in ("a", "b"):
            work[:] = src
            t0 = time.perf_counter()
            rdst_amd.sort_host_records(work, "score" if case == "a" else one)
            t1 = time.perf_counter()
            if rep:
                ms[case].append((t1 - t0) * 1e3)
            elif case not in sorted_by:
                sorted_by[case] = work["score"][:: max(1, n // 1000)].copy()
    assert np.array_equal(sorted_by["a"].view(np.uint32), sorted_by["b"].view(np.uint32))
    results["a_sort_records_f32"] = _stats(ms["a"])
    results["b_sort_records_by_fields_f32"] = _stats(ms["b"])
    results["b_over_a"] = round(results["b_sort_records_by_fields_f32"]["ms"] / results["a_sort_records_f32"]["ms"], 4)
    print(json.dumps({k: results[k] for k in ("a_sort_records_f32", "b_sort_records_by_fields_f32", "b_over_a")}), flush=True)

    # (c): device entry
    dev_src = torch.from_numpy(src.view(np.uint8).reshape(n, REC)).cuda()
    dev = torch.empty_like(dev_src)
    table2, nf2 = _field_table(two)
    scratch = torch.empty(int(lib.rdst_hip_sort_records_by_fields_scratch_bytes(n, REC, table2, nf2)), dtype=torch.uint8, device="cuda")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c_ms = []
    for rep in range(reps + 1):
        dev.copy_(dev_src)
        torch.cuda.synchronize()
        start.record()
        rdst_amd.sort_records_device_tensor(dev, two, scratch=scratch, check=False)
        stop.record()
        stop.synchronize()
        if rep:
            c_ms.append(start.elapsed_time(stop))
    rdst_amd.device_status()
    results["c_device_u16_i64"] = dict(_stats(c_ms), scratch_bytes=scratch.numel(), key_bytes=10)
    print(json.dumps({"c_device_u16_i64": results["c_device_u16_i64"]}), flush=True)

    # (d): the pack kernel alone, and the streaming copy over the same number of bytes
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, fields, key_out, rows_out in (("d_pack_f32_L4", one, 4, 4), ("d_pack_u16_i64_L10", two, 10, 0)):
        table, nf = _field_table(fields)
        keys = torch.empty(n * key_out, dtype=torch.uint8, device="cuda")
        rows = torch.empty(n, dtype=torch.int32, device="cuda")
        moved = n * (REC + key_out + rows_out)             # the staged form reads whole records
        half = moved // 2 // 16 * 16
        cp_src, cp_dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        p_ms, cp_ms = [], []
        for rep in range(reps + 1):
            start.record()
            _lib.check(lib.rdst_hip_pack_fields_device(ctypes.c_void_p(dev_src.data_ptr()), n, REC, table, nf, ctypes.c_void_p(keys.data_ptr()),
                                                       ctypes.c_void_p(rows.data_ptr()), s))
            stop.record()
            stop.synchronize()
            if rep:
                p_ms.append(start.elapsed_time(stop))
            start.record()
            _lib.check(lib.rdst_hip_stream_copy(ctypes.c_void_p(cp_dst.data_ptr()), ctypes.c_void_p(cp_src.data_ptr()), half, s))
            stop.record()
            stop.synchronize()
            if rep:
                cp_ms.append(start.elapsed_time(stop))
        rdst_amd.device_status()
        p, c = _stats(p_ms), _stats(cp_ms)
        results[name] = dict(p, bytes_read_per_record=REC, bytes_written_per_record=key_out + rows_out,
                             gb_per_s=round(moved / (p["ms"] / 1e3) / 1e9, 1),
                             stream_copy={"bytes_moved": 2 * half, "ms": c["ms"], "ms_all": c["ms_all"], "gb_per_s": round(2 * half / (c["ms"] / 1e3) / 1e9, 1)})
        print(json.dumps({name: results[name]}), flush=True)
        del keys, rows, cp_src, cp_dst

    summary = {"tool": "tools/fields_bench.py", "device": torch.cuda.get_device_name(0), "rows": n, "record_bytes": REC, "reps": reps,
               "results": results}
    print(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
