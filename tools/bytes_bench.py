"""Device-entry timings of [u8; N] sorts (rdst_hip_sort_bytes_device), one JSON line per case and a summary object.

    python tools/bytes_bench.py [--reps 5] [--scale 1.0] [--out profiles/bytes_bench.json]
    python tools/bytes_bench.py --nowait [--reps 5] [--scale 1.0] [--out profiles/bytes_nowait_bench.json]

Every case sorts a fresh copy of the same input (the copy is not timed), after one untimed warm-up sort; the time is
HIP events on the tensor's stream around the entry point, median over --reps.  The [u8; 16] case takes the widened
integer route the entry keeps for N <= 16; "pairs_u64_u32" is the stable pair sort the N > 16 route is built on, alone,
for reference.  --scale shrinks every size (smoke runs).

--nowait: every case with N > 16 runs through rdst_hip_sort_bytes_device and rdst_hip_sort_bytes_device_nowait in the same
process, alternating, each from a fresh copy; the line holds both medians and their ratio.  A random case whose ratio
exceeds 1.5 is run once more with rdst_hip_set_profiling and its pair sorts' stage times are added.  Then one flag-down
round alone at the random cases' size: the all-skipped pair sort (all-zero u64 keys, u32 values: what such a round sorts)
by HIP events, and rdst_hip_stream_fill over 8 bytes per row standing in for the chunk-key kernel, which with the flag down
reads one word and stores 8 bytes of zeros per row.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cases(scale):
    big, mid = int(1e8 * scale), int(1e7 * scale)
    return [
        ("random_u8x16", big, 16, "random"),
        ("random_u8x20", big, 20, "random"),
        ("random_u8x32", big, 32, "random"),
        ("random_u8x64", big, 64, "random"),
        ("prefix56_u8x64", mid, 64, "prefix56"),
        ("identical_u8x64", mid, 64, "identical"),
    ]


def _input(torch, n, N, shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 256, (n, N), dtype=torch.uint8, device="cuda", generator=g)
    if shape == "prefix56":
        t[:, :56] = 0x5A
    elif shape == "identical":
        t[:] = t[0]
    return t


def _time(torch, fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps + 1):
        prep = fn(None)
        torch.cuda.synchronize()
        start.record()
        fn(prep)
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    ms = sorted(ms[1:])  # the first one is the warm-up
    return ms[len(ms) // 2], ms


def _time_alternating(torch, fns, reps):
    """`fns`: name -> fn(prep) as _time takes it; one warm-up round, then --reps rounds, each running every fn once"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {name: [] for name in fns}
    for rep in range(reps + 1):
        for name, fn in fns.items():
            prep = fn(None)
            torch.cuda.synchronize()
            start.record()
            fn(prep)
            stop.record()
            stop.synchronize()
            if rep:
                ms[name].append(start.elapsed_time(stop))
    return {name: sorted(v) for name, v in ms.items()}


def _profiled(torch, rdst_amd, fn):
    """one more run of fn under rdst_hip_set_profiling: per recorded run (one per pair sort), the stage times summed by name"""
    rdst_amd.set_profiling(True)
    try:
        prep = fn(None)
        torch.cuda.synchronize()
        fn(prep)
        torch.cuda.synchronize()
        runs = []
        for r in range(rdst_amd.profile_runs()):
            got = rdst_amd.profile_run(r, 0)
            if got:
                by = {}
                for name, _level, ms in got["stages"]:
                    by[name] = round(by.get(name, 0.0) + ms, 3)
                runs.append(by)
        return runs
    finally:
        rdst_amd.set_profiling(False)


def _nowait_main(args, torch, rdst_amd, lib):
    import ctypes
    from rdst_amd._lib import check as _lib_check
    results = []
    for name, n, N, shape in _cases(args.scale):
        if N <= 16:
            continue                                        # forwarded: the same route under both names
        src = _input(torch, n, N, shape, seed=N)
        work = torch.empty_like(src)
        scratch = torch.empty(int(lib.rdst_hip_sort_bytes_scratch_bytes(n, N)), dtype=torch.uint8, device="cuda")

        def entry(sort):
            def run(prep):
                if prep is None:
                    work.copy_(src)
                    return True
                sort(work, scratch=scratch, check=False)
                return None
            return run

        fns = {"blocking": entry(rdst_amd.sort_bytes_device_tensor), "nowait": entry(rdst_amd.sort_bytes_device_nowait_tensor)}
        ms = _time_alternating(torch, fns, args.reps)
        rdst_amd.device_status()
        head = work[:2].cpu().numpy()
        assert n < 2 or bytes(head[0]) <= bytes(head[1])
        nowait_result = work.clone()                        # (the last run was the nowait entry's)
        fns["blocking"](fns["blocking"](None))
        rdst_amd.device_status()
        assert torch.equal(nowait_result, work), "the two entries disagree"
        del nowait_result
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        rec = {"case": name, "rows": n, "n_bytes": N, "rounds": -(-N // 8), "blocking_ms": round(med["blocking"], 3),
               "nowait_ms": round(med["nowait"], 3), "nowait_over_blocking": round(med["nowait"] / med["blocking"], 3),
               "blocking_ms_all": [round(x, 3) for x in ms["blocking"]], "nowait_ms_all": [round(x, 3) for x in ms["nowait"]]}
        if shape == "random" and rec["nowait_over_blocking"] > 1.5:
            rec["nowait_pair_sort_stages_ms"] = _profiled(torch, rdst_amd, fns["nowait"])
            rec["blocking_pair_sort_stages_ms"] = _profiled(torch, rdst_amd, fns["blocking"])
            rdst_amd.device_status()
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del src, work, scratch, fns
        torch.cuda.empty_cache()
    # one flag-down round alone
    n = int(1e8 * args.scale)
    keys, vals = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.arange(n, dtype=torch.int32, device="cuda")
    tk, tv = torch.empty_like(keys), torch.empty_like(vals)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def skipped(prep):
        if prep is None:
            return True
        rdst_amd.sort_pairs_device_tensor(keys, vals, tk, tv, check=False)
        return None

    def fill(prep):
        if prep is None:
            return True
        _lib_check(lib.rdst_hip_stream_fill(ctypes.c_void_p(tk.data_ptr()), n * 8 // 16 * 16, s))
        return None

    ms = _time_alternating(torch, {"pair_sort_all_levels_skipped": skipped, "fill_8_bytes_per_row": fill}, args.reps)
    rdst_amd.device_status()
    assert bool((vals[:1000] == torch.arange(1000, dtype=torch.int32, device="cuda")).all())
    med = {k: v[len(v) // 2] for k, v in ms.items()}
    rec = {"case": "flag_down_round", "rows": n, "pair_sort_all_levels_skipped_ms": round(med["pair_sort_all_levels_skipped"], 3),
           "fill_8_bytes_per_row_ms": round(med["fill_8_bytes_per_row"], 3), "round_ms": round(sum(med.values()), 3),
           "ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()}}
    print(json.dumps(rec), flush=True)
    results.append(rec)
    return {"tool": "tools/bytes_bench.py --nowait", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results}


def _write(summary, out):
    print(json.dumps(summary))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(summary, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--nowait", action="store_true", help="blocking and nowait entries alternating, case by case")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import rdst_amd
    from rdst_amd import _lib
    torch.cuda.set_device(0)
    lib = _lib.load()
    if args.nowait:
        _write(_nowait_main(args, torch, rdst_amd, lib), args.out)
        return
    results = []
    for name, n, N, shape in _cases(args.scale):
        src = _input(torch, n, N, shape, seed=N)
        work = torch.empty_like(src)
        scratch = torch.empty(int(lib.rdst_hip_sort_bytes_scratch_bytes(n, N)), dtype=torch.uint8, device="cuda")

        def run(prep, src=src, work=work, scratch=scratch):
            if prep is None:
                work.copy_(src)
                return True
            rdst_amd.sort_bytes_device_tensor(work, scratch=scratch, check=False)
            return None

        med, all_ms = _time(torch, run, args.reps)
        rdst_amd.device_status()
        head = work[:2].cpu().numpy()
        assert n < 2 or bytes(head[0]) <= bytes(head[1])
        rec = {"case": name, "rows": n, "n_bytes": N, "ms": round(med, 3), "ms_all": [round(x, 3) for x in all_ms],
               "rows_per_s": round(n / (med / 1e3)) if med > 0 else None, "gb_rows_per_s": round(n * N / (med / 1e3) / 1e9, 1) if med > 0 else None}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del src, work, scratch
        torch.cuda.empty_cache()
    # the stable pair sort alone at the random cases' size
    n = int(1e8 * args.scale)
    keys_src = torch.randint(-(2**63), 2**63 - 1, (n,), dtype=torch.int64, device="cuda")
    keys, vals = torch.empty_like(keys_src), torch.empty(n, dtype=torch.int32, device="cuda")
    tk, tv = torch.empty_like(keys), torch.empty_like(vals)
    ar = torch.arange(n, dtype=torch.int32, device="cuda")

    def pairs(prep):
        if prep is None:
            keys.copy_(keys_src)
            vals.copy_(ar)
            return True
        rdst_amd.sort_pairs_device_tensor(keys, vals, tk, tv, check=False)
        return None

    med, all_ms = _time(torch, pairs, args.reps)
    rdst_amd.device_status()
    rec = {"case": "pairs_u64_u32", "rows": n, "ms": round(med, 3), "ms_all": [round(x, 3) for x in all_ms]}
    print(json.dumps(rec), flush=True)
    results.append(rec)
    _write({"tool": "tools/bytes_bench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results}, args.out)


if __name__ == "__main__":
    main()
