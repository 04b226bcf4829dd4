"""Device timings of the runs of equal keys (rdst_hip_runs_device) beside the floors of a pass that reads its input once and
beside what a caller paid before.  One JSON line per case and a summary object.

    python tools/runs_bench.py [--reps 7] [--scale 1.0] [--out profiles/runs_bench.json] [--ab LIB_A LIB_B [--ab-rounds 4]]

Inputs: 10^8 and 10^9 u32 keys, 10^9 u64 keys, 10^8 u128 keys (--scale shrinks them), each all distinct and sorted, in runs
of 16, in runs of 4 096 and all equal.  Per input, in one process, alternating after an untimed warm-up round, HIP events on the
stream around each call, median over --reps with every time kept:
  runs        the call at capacity = len with keys, 8-byte starts and the count
  runs_pad    the same with RDST_RUNS_PAD_STARTS (a second launch that writes (R, len])
  read        rdst_hip_stream_read of the input's bytes: the floor of a pass that reads once
  copy        (all distinct only) rdst_hip_stream_copy of (bytes read + bytes written) / 2 bytes, i.e. the same traffic
  torch       torch.unique_consecutive(return_counts=True) and the synchronise it ends in (no 16-byte keys)
`bytes_read` / `bytes_written` are computed from the shapes.  --ab runs bench.py's headline in child processes on two builds of
the library, alternating, and records both series."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("u32", 4, 10**8), ("u32", 4, 10**9), ("u64", 8, 10**9), ("u128", 16, 10**8))
SHAPES = (("all_distinct", 1), ("runs_of_16", 16), ("runs_of_4096", 4096), ("all_equal", 0))


def _time_alternating(torch, fns, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {name: [] for name in fns}
    for rep in range(reps + 1):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if rep:
                ms[name].append(start.elapsed_time(stop))
    return {name: sorted(v) for name, v in ms.items()}


def _keys(torch, key, n, run):
    """sorted keys in runs of `run` (0: all equal): run index r as the key; u128: limbs [low = r, high = 0]"""
    r = torch.arange(n, dtype=torch.int64, device="cuda")
    r = r // run if run else r * 0 + 7
    if key == "u32":
        return r.to(torch.int32).view(torch.uint32)
    if key == "u64":
        return r.view(torch.uint64)
    return torch.stack([r, torch.zeros_like(r)], dim=1).contiguous()


def _median(v):
    return v[len(v) // 2] if v else None


def _ab(libs, rounds, steps, warmup):
    # (an older build lacks the newest symbols: the binding leaves out what the library does not export)
    code = ("import sys, runpy, ctypes, torch\nsys.path.insert(0, %r)\nfrom rdst_amd import _lib\n_lib.LIB_PATH = %r\n"
            "probe = ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)\n"
            "for name in [n for n in _lib.SIGNATURES if not hasattr(probe, n)]:\n    del _lib.SIGNATURES[name]\n"
            "sys.argv = ['bench.py', '--gpus', '1', '--steps', %r, '--warmup', %r]\nrunpy.run_path(%r, run_name='__main__')\n")
    series = {lib: [] for lib in libs}
    for _ in range(rounds):
        for lib in libs:
            out = subprocess.run([sys.executable, "-c", code % (ROOT, os.path.abspath(lib), str(steps), str(warmup), os.path.join(ROOT, "bench.py"))],
                                 capture_output=True, text=True, timeout=600)
            lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
            if out.returncode != 0 or not lines:
                raise SystemExit(f"bench.py failed on {lib}: {out.stderr[-800:]}")
            series[lib].append(json.loads(lines[-1])["value"])
            print(json.dumps({"ab": lib, "value": series[lib][-1]}), flush=True)
    return series


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab", nargs=2, default=None, metavar="LIB", help="two builds of the library: bench.py's headline on each, alternating")
    ap.add_argument("--ab-rounds", type=int, default=4)
    ap.add_argument("--only-ab", action="store_true")
    args = ap.parse_args()
    import torch
    import rdst_amd
    from rdst_amd import _lib
    assert torch.cuda.is_available(), "no HIP device: nothing is measured without one"
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    cases = []
    for key, kb, n in (() if args.only_ab else CASES):
        n = max(4096, int(n * args.scale))
        wide = key if key == "u128" else None
        for shape, run in SHAPES:
            keys = _keys(torch, key, n, run)
            out = (torch.empty_like(keys), torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda"))
            scratch = torch.empty(rdst_amd.runs_scratch_bytes(n, {"u32": "uint32", "u64": "uint64"}.get(key, key)), dtype=torch.uint8, device="cuda")
            runs = n if run == 1 else (1 if run == 0 else -(-n // run))
            read, written = n * kb, runs * (kb + 8) + 16
            half = (read + written) // 2 // 16 * 16
            fns = {"runs": lambda: rdst_amd.runs_device_tensor(keys, scratch=scratch, check=False, key=wide, out=out),
                   "runs_pad": lambda: rdst_amd.runs_device_tensor(keys, pad=True, scratch=scratch, check=False, key=wide, out=out),
                   "read": lambda: _lib.check(lib.rdst_hip_stream_read(keys.data_ptr(), n * kb // 16 * 16, stream))}
            if run == 1:
                src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
                fns["copy"] = lambda: _lib.check(lib.rdst_hip_stream_copy(dst.data_ptr(), src.data_ptr(), half, stream))
            if key != "u128":
                signed = keys.view(torch.int32 if kb == 4 else torch.int64)

                def torch_way():
                    u, c = torch.unique_consecutive(signed, return_counts=True)
                    torch.cuda.synchronize()
                    return u, c
                fns["torch"] = torch_way
            ms = _time_alternating(torch, fns, args.reps)
            rdst_amd.device_status()
            assert int(out[2].item()) == runs and int(out[1][runs].item()) == n and int(out[1][min(runs, n) - 1].item()) == (runs - 1) * max(run, 1) * (run != 0)
            med = {name: _median(v) for name, v in ms.items()}
            case = {"key": key, "n": n, "shape": shape, "runs": runs, "bytes_read": read, "bytes_written": written, "ms": ms, "median_ms": med,
                    "read_over_runs": med["read"] / med["runs"], "gb_per_s": (read + written) / med["runs"] / 1e6}
            if "copy" in med:
                case["copy_over_runs"] = med["copy"] / med["runs"]
            if "torch" in med:
                case["torch_over_runs"] = med["torch"] / med["runs"]
            print(json.dumps(case), flush=True)
            cases.append(case)
            del keys, out, scratch, fns
            torch.cuda.empty_cache()
    summary = {"tool": "tools/runs_bench.py", "reps": args.reps, "scale": args.scale, "cases": cases}
    if args.ab:
        summary["bench_ab"] = {"unit": "Gkeys/s (bench.py --gpus 1 --steps 6 --warmup 2)", "series": _ab(args.ab, args.ab_rounds, 6, 2)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    print(json.dumps({k: v for k, v in summary.items() if k != "cases"}))


if __name__ == "__main__":
    main()
