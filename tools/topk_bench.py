"""Device timings of the partial sort (rdst_hip_topk_device) against what the library offered for the same result before it
— a device copy of the keys (the sort is in place), rdst_hip_sort_device on the copy (with an index: an iota and
rdst_hip_sort_pairs_device), the first k elements — and, for information only, torch.topk.  One JSON line per case and a
summary object.

    python tools/topk_bench.py [--reps 5] [--scale 1.0] [--out profiles/topk_bench.json]

Inputs: u32, u64 and (u32, index) with uniform keys, an f32 column of normal values, u32 keys that are all equal;
n = 10^8 and 10^9 (--scale shrinks both); k = 1, 10^3, 10^6.  The candidates run in the same process, alternating, after one
untimed warm-up round; the time is HIP events on the stream around the calls, median over --reps with all of them kept.
Every case's result is compared with the baseline's first k.  One more run of the partial sort under
rdst_hip_set_profiling gives the time of every select level (levels the device did not need show what a launch that returns
at once costs) and of the collection pass."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def _levels_profile(torch, rdst_amd, fn):
    """(per-level ms, collection ms) of one profiled run of the partial sort"""
    rdst_amd.set_profiling(True)
    try:
        fn()
        torch.cuda.synchronize()
        levels, collect = [], None
        for r in range(rdst_amd.profile_runs()):
            got = rdst_amd.profile_run(r, 0)
            for name, level, ms in (got["stages"] if got else ()):
                if name == "topk" and level == 255:
                    collect = round(ms, 4)
                elif name == "topk":
                    levels.append(round(ms, 4))
        return levels, collect
    finally:
        rdst_amd.set_profiling(False)


def _inputs(torch, n, seed):
    """name -> (keys tensor, indexed)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    yield "u32_uniform", torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=g).view(torch.uint32), False
    yield "u64_uniform", torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=g).view(torch.uint64), False
    yield "u32_uniform_indexed", torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=g).view(torch.uint32), True
    yield "f32_normal", torch.randn(n, dtype=torch.float32, device="cuda", generator=g), False
    yield "u32_all_equal", torch.full((n,), 0x12345678, dtype=torch.int32, device="cuda").view(torch.uint32), False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch.topk column out")
    args = ap.parse_args()
    import torch
    import rdst_amd
    torch.cuda.set_device(0)
    results = []
    for n in (int(1e8 * args.scale), int(1e9 * args.scale)):
        for name, keys, indexed in _inputs(torch, n, 1 + n % 7):
            copy, tmp = torch.empty_like(keys), torch.empty_like(keys)
            vals = tmp_vals = None
            if indexed:
                vals, tmp_vals = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
            signed = keys.view(torch.int32 if keys.element_size() == 4 else torch.int64) if not keys.dtype.is_floating_point else keys
            for k in (1, 1000, 1_000_000):
                if k > n:
                    continue
                ib = 4 if indexed else 0
                scratch = torch.empty(rdst_amd.topk_scratch_bytes(n, k, keys.dtype, ib), dtype=torch.uint8, device="cuda")
                out = {}

                def topk():
                    out["topk"] = rdst_amd.topk_device_tensor(keys, k, index=torch.int32 if indexed else None, scratch=scratch, check=False)

                def baseline():
                    copy.copy_(keys)
                    if indexed:
                        torch.arange(n, dtype=torch.int32, device="cuda", out=vals)
                        rdst_amd.sort_pairs_device_tensor(copy, vals, tmp, tmp_vals, check=False)
                    else:
                        rdst_amd.sort_device_tensor(copy, tmp, check=False)

                fns = {"topk": topk, "baseline": baseline}
                if not args.no_torch:
                    # torch.topk has no unsigned kernels: integer keys go in as the same bits, signed (another order, the same
                    # work; for information only)
                    fns["torch_topk"] = lambda: torch.topk(signed, k, largest=False, sorted=True)
                try:
                    ms = _time_alternating(torch, fns, args.reps)
                except RuntimeError as e:                   # (torch.topk may not take the size: the column is information only)
                    if "torch_topk" not in fns:
                        raise
                    del fns["torch_topk"]
                    torch.cuda.synchronize()
                    ms = _time_alternating(torch, fns, args.reps)
                    ms["torch_topk"] = []
                    print(f"# torch.topk left out for {name} n = {n} k = {k}: {str(e)[:100]}", flush=True)
                rdst_amd.device_status()
                baseline()
                topk()
                rdst_amd.device_status()
                got_k, got_i = out["topk"]
                assert torch.equal(got_k.view(torch.uint8), copy[:k].view(torch.uint8)), "the partial sort and the baseline disagree"
                if indexed:
                    assert torch.equal(got_i, vals[:k]), "the positions disagree"
                state = rdst_amd.topk_state(scratch)
                levels_ms, collect_ms = _levels_profile(torch, rdst_amd, topk)
                med = {name_: (v[len(v) // 2] if v else None) for name_, v in ms.items()}
                rec = {"case": name, "n": n, "k": k, "topk_ms": round(med["topk"], 4), "baseline_ms": round(med["baseline"], 4),
                       "baseline_over_topk": round(med["baseline"] / med["topk"], 2),
                       "torch_topk_ms": round(med["torch_topk"], 4) if med.get("torch_topk") is not None else None,
                       "topk_spread": round(ms["topk"][-1] / ms["topk"][0], 3), "baseline_spread": round(ms["baseline"][-1] / ms["baseline"][0], 3),
                       "topk_ms_all": [round(x, 4) for x in ms["topk"]], "baseline_ms_all": [round(x, 4) for x in ms["baseline"]],
                       "levels_used": state["levels"], "candidates": state["candidates"], "c_below": state["c_below"], "special": state["special"],
                       "level_ms": levels_ms, "collect_ms": collect_ms, "results_equal": True}
                print(json.dumps(rec), flush=True)
                results.append(rec)
                del scratch, out
            del keys, copy, tmp, vals, tmp_vals, signed
            torch.cuda.empty_cache()
        rdst_amd.release_workspace()
    # what a launch pair (count + pick) that returns at once costs: the levels behind the last one used
    idle = [ms for r in results for ms in r["level_ms"][r["levels_used"]:]]
    summary = {"tool": "tools/topk_bench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps,
               "idle_level_ms_median": round(sorted(idle)[len(idle) // 2], 4) if idle else None,
               "slower_than_baseline": [[r["case"], r["n"], r["k"]] for r in results if r["topk_ms"] > r["baseline_ms"]], "results": results}
    print(json.dumps({k: v for k, v in summary.items() if k != "results"}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
