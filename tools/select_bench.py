"""Device timings of the order statistics (rdst_hip_select_device) against what the library offered for the same result
before it — (a) a device copy of the keys (the sort is in place), rdst_hip_sort_device on the copy (with an index: an iota and
rdst_hip_sort_pairs_device) and a gather at the ranks; (b) rdst_hip_topk_device with k = the largest rank + 1, where that k
is at most 10^6 — and, for information only, torch.kthvalue (one call, one rank) and torch.quantile where it takes the size.
One JSON line per case and a summary object.

    python tools/select_bench.py [--reps 7] [--scale 1.0] [--out profiles/select_bench.json] [--no-torch] [--no-sweep]
                                 [--ranks median,deciles,spaced]

Inputs: u32, u64 and (u32, int32 index) with uniform keys, an f32 column of normal values; u32 keys all equal and u32 keys
already sorted; n = 10^8 and 10^9 (--scale shrinks both).  Rank sets: the median alone, the nine deciles, max_ranks evenly
spaced ranks; with --ranks low also the 0.01 % quantile alone (rank n / 10^4: the one set whose k is small enough for
yardstick (b)).  The candidates run in the same process, alternating, after one untimed warm-up round; the time is HIP events on
the stream around the calls, median over --reps with all of them kept.  Every case's result is compared with the baseline's
elements at the ranks.  `reads` is the number of times the call read the input: the levels it used and the collection (none
when the digits were exhausted).  The sweep times the uniform u32 column at max_ranks ranks over cand_capacity: the default
must hold one level's groups."""
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


def _inputs(torch, rdst_amd, n, seed):
    """name -> (keys tensor, indexed)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)

    def u32():
        return torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=g).view(torch.uint32)

    yield "u32_uniform", u32(), False
    yield "u64_uniform", torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=g).view(torch.uint64), False
    yield "f32_normal", torch.randn(n, dtype=torch.float32, device="cuda", generator=g), False
    yield "u32_uniform_indexed", u32(), True
    yield "u32_all_equal", torch.full((n,), 0x12345678, dtype=torch.int32, device="cuda").view(torch.uint32), False
    s = u32()
    rdst_amd.sort_device_tensor(s)
    yield "u32_sorted", s, False


def _rank_sets(rdst_amd, n, max_ranks, names=("median", "deciles", "spaced")):
    sets = {"median": rdst_amd.quantile_ranks(n, [0.5]), "deciles": rdst_amd.quantile_ranks(n, [i / 10 for i in range(1, 10)]),
            "spaced": [int((2 * i + 1) * n // (2 * max_ranks)) for i in range(max_ranks)], "low": rdst_amd.quantile_ranks(n, [1e-4])}
    return tuple((name, sets[name]) for name in names)


def _median(v):
    return v[len(v) // 2] if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch.kthvalue / torch.quantile columns out")
    ap.add_argument("--no-sweep", action="store_true", help="leave the cand_capacity sweep out")
    ap.add_argument("--ranks", default="median,deciles,spaced", help="the rank sets, of median, deciles, spaced, low")
    args = ap.parse_args()
    import torch
    import rdst_amd
    torch.cuda.set_device(0)
    results, sweep = [], []
    for n in (int(1e8 * args.scale), int(1e9 * args.scale)):
        for name, keys, indexed in _inputs(torch, rdst_amd, n, 1 + n % 7):
            ib = 4 if indexed else 0
            max_ranks, _d0, _d, default_cap, _lv = rdst_amd.select_limits(keys.dtype, ib)
            copy, tmp = torch.empty_like(keys), torch.empty_like(keys)
            vals = tmp_vals = None
            if indexed:
                vals, tmp_vals = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
            def as_signed(t):                           # (torch gathers and selects signed integers only: the same bits)
                return t if t.dtype.is_floating_point else t.view(torch.int32 if t.element_size() == 4 else torch.int64)

            signed = as_signed(keys)
            scratch = torch.empty(rdst_amd.select_scratch_bytes(n, max_ranks, keys.dtype, ib), dtype=torch.uint8, device="cuda")
            for set_name, ranks in _rank_sets(rdst_amd, n, max_ranks, tuple(args.ranks.split(","))):
                at = torch.tensor(ranks, dtype=torch.int64, device="cuda")
                out = {}

                def select():
                    out["select"] = rdst_amd.select_device_tensor(keys, ranks, index=torch.int32 if indexed else None, scratch=scratch, check=False)

                def baseline():
                    copy.copy_(keys)
                    if indexed:
                        torch.arange(n, dtype=torch.int32, device="cuda", out=vals)
                        rdst_amd.sort_pairs_device_tensor(copy, vals, tmp, tmp_vals, check=False)
                        out["baseline"] = (as_signed(copy)[at], vals[at])
                    else:
                        rdst_amd.sort_device_tensor(copy, tmp, check=False)
                        out["baseline"] = (as_signed(copy)[at], None)

                fns = {"select": select, "baseline": baseline}
                k = max(ranks) + 1
                if k <= 1_000_000:
                    topk_scratch = torch.empty(rdst_amd.topk_scratch_bytes(n, k, keys.dtype, ib), dtype=torch.uint8, device="cuda")
                    fns["topk"] = lambda: rdst_amd.topk_device_tensor(keys, k, index=torch.int32 if indexed else None, scratch=topk_scratch, check=False)
                ms = _time_alternating(torch, fns, args.reps)
                extra = {}
                if not args.no_torch and set_name in ("median", "low"):
                    # torch has no unsigned kernels: integer keys go in as the same bits, signed (another order, the same work)
                    for tname, fn in (("torch_kthvalue", lambda: torch.kthvalue(signed, ranks[0] + 1)),
                                      ("torch_quantile", lambda: torch.quantile(signed, 0.5, interpolation="lower"))):
                        try:
                            extra[tname + "_ms"] = round(_median(_time_alternating(torch, {tname: fn}, 3)[tname]), 4)
                        except (RuntimeError, TypeError) as e:
                            extra[tname + "_ms"] = None
                            extra[tname + "_refused"] = str(e)[:80]
                            torch.cuda.synchronize()
                rdst_amd.device_status()
                baseline()
                select()
                rdst_amd.device_status()
                got_k, got_i = out["select"]
                assert torch.equal(got_k.view(torch.uint8), out["baseline"][0].view(torch.uint8)), "the select and the baseline disagree"
                if indexed:
                    assert torch.equal(got_i, out["baseline"][1]), "the positions disagree"
                state = rdst_amd.select_state(scratch)
                med = {name_: _median(v) for name_, v in ms.items()}
                rec = {"case": name, "n": n, "ranks": set_name, "n_ranks": len(ranks), "select_ms": round(med["select"], 4),
                       "baseline_ms": round(med["baseline"], 4), "baseline_over_select": round(med["baseline"] / med["select"], 2),
                       "topk_ms": round(med["topk"], 4) if "topk" in med else None,
                       "topk_over_select": round(med["topk"] / med["select"], 2) if "topk" in med else None,
                       "select_ms_all": [round(x, 4) for x in ms["select"]], "baseline_ms_all": [round(x, 4) for x in ms["baseline"]],
                       "levels_used": state["levels"], "groups": state["groups"], "candidates": state["candidates"], "exhausted": state["exhausted"],
                       "reads": state["levels"] + (0 if state["exhausted"] else 1), "results_equal": True, **extra}
                print(json.dumps(rec), flush=True)
                results.append(rec)
            if name == "u32_uniform" and not args.no_sweep:
                ranks = _rank_sets(rdst_amd, n, max_ranks, ("spaced",))[0][1]
                for cap in (1 << 12, 1 << 16, 1 << 20, 1 << 22, default_cap, 1 << 26):
                    sc = torch.empty(rdst_amd.select_scratch_bytes(n, max_ranks, keys.dtype, 0, cap), dtype=torch.uint8, device="cuda")
                    ms = _time_alternating(torch, {"select": lambda: rdst_amd.select_device_tensor(keys, ranks, scratch=sc, cand_capacity=cap, check=False)},
                                           args.reps)["select"]
                    st = rdst_amd.select_state(sc)
                    rec = {"sweep": name, "n": n, "n_ranks": len(ranks), "cand_capacity": cap, "select_ms": round(_median(ms), 4),
                           "select_ms_all": [round(x, 4) for x in ms], "levels_used": st["levels"], "candidates": st["candidates"]}
                    print(json.dumps(rec), flush=True)
                    sweep.append(rec)
                    del sc
            del keys, copy, tmp, vals, tmp_vals, signed, scratch
            torch.cuda.empty_cache()
        rdst_amd.release_workspace()
    summary = {"tool": "tools/select_bench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "scale": args.scale,
               "rank_sets": args.ranks, "slower_than_baseline": [[r["case"], r["n"], r["ranks"]] for r in results if r["select_ms"] > r["baseline_ms"]],
               "within_spread_of_baseline": [[r["case"], r["n"], r["ranks"]] for r in results
                                             if r["select_ms"] <= r["baseline_ms"] and r["select_ms_all"][-1] >= r["baseline_ms_all"][0]],
               "results": results, "cand_capacity_sweep": sweep}
    print(json.dumps({k: v for k, v in summary.items() if k not in ("results", "cand_capacity_sweep")}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
