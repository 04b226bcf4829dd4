"""Device timings of the segmented select (rdst_hip_select_segments_device) against the two ways the library offered the same
result before it, and — for information only — torch.median(dim=1) / torch.kthvalue(dim=1).  One JSON line per case and a
summary object.

    python tools/select_segments_bench.py [--reps 7] [--scale 1.0] [--out profiles/select_segments_bench.json]
    python tools/select_segments_bench.py --stream-max-sweep [--reps 7] [--out profiles/select_segments_bench.json]
    python tools/select_segments_bench.py --device-offsets [--reps 7] [--out profiles/select_segments_offsets_bench.json]

table   rows x row length 65 536 x 64, 4 096 x 4 096, 1 024 x 16 384, 64 x 131 072, 8 x 2^20 and a ragged table of 300 rows
        with lengths from 1 to 2^18; rank sets: the median, the nine deciles, 32 ranks (quantiles i / 31); u32, f32 and u64
        keys only, f32 with an int32 index.  Baselines, existing code of the same build:
          sort    a copy of the array, the segmented sort of the copy (with an index: the segmented pair sort against a
                  per-row iota), a gather of the ranks;
          loop    select_device_tensor per row.  At most --loop-rows rows are timed and the time is scaled to the table: the
                  cost is a per-call floor, row after row (loop_rows_timed says how many ran).
--stream-max-sweep   one segment per call, lengths 2^15 .. 2^22, u32 and u64 keys, the median and the nine deciles: the stream
        class forced against the far class forced, both through rdst_hip_set_topk_segments_stream_max — the border was
        measured for top-k, and this says where it would belong for selects.
--device-offsets     rdst_hip_select_segments_device_offsets, both modes, over the same tables and rank sets and one row of
        2^24 keys, the table of borders a device tensor.  The baseline is what such a caller paid before the entry: the table
        copied to the host, a synchronise, rdst_hip_select_segments_device.

The candidates run in one process, alternating, after one untimed warm-up round; the time is HIP events on the stream around
the calls, median over --reps with all of them kept.  Every result is compared with the sort baseline's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RANK_SETS = {"median": [(1, 2)], "deciles": [(i, 10) for i in range(1, 10)], "32_ranks": [(i, 31) for i in range(32)]}


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


def _stats(v):
    return {"ms": round(v[len(v) // 2], 4), "spread": round(v[-1] / v[0], 3), "all": [round(x, 4) for x in v]}


def _keys(torch, kind, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    if kind == "f32":
        return torch.randn(n, dtype=torch.float32, device="cuda", generator=g)
    if kind == "u64":
        return torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=g).view(torch.uint64)
    return torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=g).view(torch.uint32)


def _tables(scale):
    rng = np.random.default_rng(5)
    for rows, cols in ((65536, 64), (4096, 4096), (1024, 16384), (64, 131072), (8, 1 << 20)):
        rows = max(1, int(rows * scale))
        yield f"{rows}x{cols}", np.arange(rows + 1, dtype=np.uint64) * np.uint64(cols), cols
    lengths = np.concatenate([[1, 1 << 18], (2.0 ** rng.uniform(0, 18, size=max(2, int(298 * scale)))).astype(np.int64)])
    yield f"ragged_{len(lengths)}_rows_1_to_2^18", np.concatenate([[0], np.cumsum(rng.permutation(lengths))]).astype(np.uint64), None


def _resolved(rdst_amd, lens, quantiles):
    """(n_segments, n_ranks) ranks, lower method; -1 where a segment has none"""
    cache = {}
    out = np.full((len(lens), len(quantiles)), -1, dtype=np.int64)
    for s, n in enumerate(lens.tolist()):
        if n not in cache:
            cache[n] = [rdst_amd.rank_for_length(n, quantile=q) for q in quantiles]
        out[s] = [-1 if r is None else r for r in cache[n]]
    return out


def table(torch, rdst_amd, args):
    results = []
    for shape, off, cols in _tables(args.scale):
        n, n_seg = int(off[-1]), len(off) - 1
        lens = (off[1:] - off[:-1]).astype(np.int64)
        longest = int(lens.max())
        for kind, indexed in (("u32", False), ("f32", False), ("u64", False), ("f32", True)):
            keys = _keys(torch, kind, n, n_seg % 11 + len(kind))
            ib = 4 if indexed else 0
            index = torch.int32 if indexed else None
            _wm, bm, sm, _mr = rdst_amd.select_segments_limits(keys.dtype, ib)
            sort_bm = rdst_amd.segments_limits(keys.dtype, ib)[1]
            copy = torch.empty_like(keys)
            tmp = torch.empty(longest, dtype=keys.dtype, device="cuda") if longest > sort_bm else None
            iota_src = vals = tmp_vals = None
            if indexed:
                starts = torch.from_numpy(np.repeat(off[:-1].astype(np.int64), lens)).cuda()
                iota_src = (torch.arange(n, dtype=torch.int64, device="cuda") - starts).to(torch.int32)   # the per-row iota, made once
                vals = torch.empty_like(iota_src)
                tmp_vals = torch.empty(longest, dtype=torch.int32, device="cuda") if longest > sort_bm else None
                del starts
            signed = keys if keys.dtype.is_floating_point else keys.view(torch.int32 if keys.element_size() == 4 else torch.int64)
            for set_name, quantiles in RANK_SETS.items():
                nr = len(quantiles)
                ranks = _resolved(rdst_amd, lens, quantiles)                # every segment here has at least one key: all resolve
                src_at = torch.from_numpy((off[:-1].astype(np.int64)[:, None] + ranks).reshape(-1)).cuda()
                scratch = torch.empty(rdst_amd.select_segments_scratch_bytes(n_seg, longest, nr, keys.dtype, ib), dtype=torch.uint8, device="cuda")
                out_k = torch.zeros((n_seg, nr), dtype=keys.dtype, device="cuda")
                out_i = torch.zeros((n_seg, nr), dtype=torch.int32, device="cuda") if indexed else None
                base_k, base_i = torch.zeros_like(out_k), (torch.zeros_like(out_i) if indexed else None)
                loop_rows = min(n_seg, args.loop_rows)
                loop_scratch = torch.empty(max(rdst_amd.select_scratch_bytes(longest, nr, keys.dtype, ib), 256), dtype=torch.uint8, device="cuda")
                row_ranks = [ranks[s].tolist() for s in range(loop_rows)]

                def segments():
                    rdst_amd.select_segments_device_tensor(keys, off, quantiles=quantiles, index=index, scratch=scratch, check=False, out=(out_k, out_i))

                def loop():
                    for s in range(loop_rows):
                        rdst_amd.select_device_tensor(keys[int(off[s]):int(off[s + 1])], row_ranks[s], index=index, scratch=loop_scratch, check=False)

                def sort():
                    copy.copy_(keys)
                    if indexed:
                        vals.copy_(iota_src)
                        rdst_amd.sort_segments_device_tensor(copy, off, tmp=tmp, values=vals, tmp_values=tmp_vals, check=False)
                        base_i.view(-1).copy_(vals[src_at])
                    else:
                        rdst_amd.sort_segments_device_tensor(copy, off, tmp=tmp, check=False)
                    base_k.view(torch.uint8).view(signed.dtype).view(-1).copy_(copy.view(signed.dtype)[src_at])

                fns = {"segments": segments, "loop": loop, "sort": sort}
                if cols is not None and not args.no_torch:
                    if set_name == "median":
                        fns["torch"] = lambda: torch.median(signed.view(n_seg, cols), dim=1)
                    else:                                                   # kthvalue takes one k: a call per rank
                        fns["torch"] = lambda: [torch.kthvalue(signed.view(n_seg, cols), int(r) + 1, dim=1) for r in ranks[0]]
                ms = _time_alternating(torch, fns, args.reps)
                rdst_amd.device_status()
                assert torch.equal(out_k.view(torch.uint8), base_k.view(torch.uint8)), "the segmented select and the sort baseline disagree"
                if indexed:
                    assert torch.equal(out_i, base_i), "the positions disagree"
                med = {name: v[len(v) // 2] for name, v in ms.items()}
                loop_ms = med["loop"] * n_seg / loop_rows
                counts = rdst_amd.topk_segments_plan(off, n, 1, keys.dtype, ib)[1]
                rec = {"part": "table", "shape": shape, "segments": n_seg, "n": n, "keys": kind, "index": ib, "ranks": set_name, "n_ranks": nr,
                       "class_counts": list(counts), "segments_call": _stats(ms["segments"]), "sort_baseline": _stats(ms["sort"]),
                       "loop_baseline_ms": round(loop_ms, 3), "loop_rows_timed": loop_rows, "loop_spread": round(ms["loop"][-1] / ms["loop"][0], 3),
                       "torch_ms": round(med["torch"], 4) if "torch" in med else None,
                       "sort_over_segments": round(med["sort"] / med["segments"], 2), "loop_over_segments": round(loop_ms / med["segments"], 2),
                       "results_equal": True}
                print(json.dumps(rec), flush=True)
                results.append(rec)
                del scratch, out_k, out_i, base_k, base_i, src_at, loop_scratch
            del keys, copy, tmp, iota_src, vals, tmp_vals, signed
            torch.cuda.empty_cache()
    return results


def stream_max_sweep(torch, rdst_amd, args):
    results = []
    for kind in ("u32", "u64"):
        for e in range(15, 23):
            n = 1 << e
            keys = _keys(torch, kind, n, e)
            off = np.array([0, n], dtype=np.uint64)
            for set_name in ("median", "deciles"):
                quantiles = RANK_SETS[set_name]
                rdst_amd.set_topk_segments_stream_max(1)
                scratch = torch.empty(rdst_amd.select_segments_scratch_bytes(1, n, len(quantiles), keys.dtype), dtype=torch.uint8, device="cuda")
                out = {}

                def run(border, name):
                    rdst_amd.set_topk_segments_stream_max(border)
                    out[name] = rdst_amd.select_segments_device_tensor(keys, off, quantiles=quantiles, scratch=scratch, check=False)[0]

                ms = _time_alternating(torch, {"stream": lambda: run(1 << 24, "stream"), "far": lambda: run(1, "far")}, args.reps)
                rdst_amd.device_status()
                assert torch.equal(out["stream"].view(torch.uint8), out["far"].view(torch.uint8)), "stream and far class disagree"
                rec = {"part": "stream_max_sweep", "keys": kind, "n": n, "ranks": set_name, "stream": _stats(ms["stream"]), "far": _stats(ms["far"]),
                       "far_over_stream": round(ms["far"][len(ms["far"]) // 2] / ms["stream"][len(ms["stream"]) // 2], 3)}
                print(json.dumps(rec), flush=True)
                results.append(rec)
    rdst_amd.set_topk_segments_stream_max(0)
    return results


def device_offsets(torch, rdst_amd, args):
    results = []
    tables = list(_tables(args.scale)) + [("1x16777216", np.array([0, 1 << 24], dtype=np.uint64), 1 << 24)]
    for shape, off, _cols in tables:
        n, n_seg = int(off[-1]), len(off) - 1
        longest = int((off[1:] - off[:-1]).max())
        toff = torch.from_numpy(off.astype(np.int64)).cuda()
        for kind, indexed in (("u32", False), ("f32", False), ("u64", False), ("f32", True)):
            keys = _keys(torch, kind, n, n_seg % 11 + len(kind))
            ib = 4 if indexed else 0
            index = torch.int32 if indexed else None
            for set_name, quantiles in RANK_SETS.items():
                nr = len(quantiles)
                host_scratch = torch.empty(rdst_amd.select_segments_scratch_bytes(n_seg, longest, nr, keys.dtype, ib), dtype=torch.uint8, device="cuda")
                scratch = torch.empty(rdst_amd.select_segments_device_offsets_scratch_bytes(n_seg, n, nr, keys.dtype, ib), dtype=torch.uint8, device="cuda")
                outs = {name: (torch.zeros((n_seg, nr), dtype=keys.dtype, device="cuda"),
                               torch.zeros((n_seg, nr), dtype=torch.int32, device="cuda") if indexed else None) for name in ("baseline", "async", "wait")}

                def baseline():
                    host = toff.cpu().numpy().astype(np.uint64)             # the copy and the synchronise
                    rdst_amd.select_segments_device_tensor(keys, host, quantiles=quantiles, index=index, scratch=host_scratch, check=False,
                                                           out=outs["baseline"])

                def run_async():
                    rdst_amd.select_segments_device_offsets_tensor(keys, toff, quantiles=quantiles, index=index, scratch=scratch, check=False,
                                                                   out=outs["async"])

                def run_wait():
                    rdst_amd.select_segments_device_offsets_tensor(keys, toff, quantiles=quantiles, index=index, scratch=scratch, far_capacity=n,
                                                                   check=False, out=outs["wait"])

                ms = _time_alternating(torch, {"baseline": baseline, "async": run_async, "wait": run_wait}, args.reps)
                rdst_amd.device_status()
                for name in ("async", "wait"):
                    assert torch.equal(outs[name][0].view(torch.uint8), outs["baseline"][0].view(torch.uint8)), f"{name} and the host-table entry disagree"
                    assert not indexed or torch.equal(outs[name][1], outs["baseline"][1]), f"{name}: the positions disagree"
                med = {name: v[len(v) // 2] for name, v in ms.items()}
                rec = {"part": "device_offsets", "shape": shape, "segments": n_seg, "n": n, "keys": kind, "index": ib, "ranks": set_name, "n_ranks": nr,
                       "class_counts_wait": list(rdst_amd.topk_segments_plan(off, n, 1, keys.dtype, ib)[1]),
                       "baseline_copy_sync_host_entry": _stats(ms["baseline"]), "async": _stats(ms["async"]), "wait": _stats(ms["wait"]),
                       "baseline_over_async": round(med["baseline"] / med["async"], 3), "baseline_over_wait": round(med["baseline"] / med["wait"], 3),
                       "results_equal": True}
                print(json.dumps(rec), flush=True)
                results.append(rec)
                del host_scratch, scratch, outs
            del keys
            torch.cuda.empty_cache()
    return results


def slower_lists(rows):
    """the cases of the table where the entry's median is above a baseline's, by the unrounded ms (a ratio that rounds to 1.0
    may still be a loss): (slower than sort, slower than loop), each [shape, keys, index, ranks, baseline / entry]"""
    out = ([], [])
    for r in rows:
        seg = r["segments_call"]["ms"]
        for which, base in ((0, r["sort_baseline"]["ms"]), (1, r["loop_baseline_ms"])):
            if base < seg:
                out[which].append([r["shape"], r["keys"], r["index"], r["ranks"], round(base / seg, 3)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the row counts of the table")
    ap.add_argument("--loop-rows", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch.median / torch.kthvalue column out")
    ap.add_argument("--stream-max-sweep", action="store_true", help="one segment per call: the stream class against the far class, by length")
    ap.add_argument("--device-offsets", action="store_true", help="the entry with the borders in device memory, both modes, against copy + synchronise + host entry")
    args = ap.parse_args()
    import torch
    import rdst_amd
    torch.cuda.set_device(0)
    summary = {"tool": "tools/select_segments_bench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps,
               "limits_u32": rdst_amd.select_segments_limits("uint32"), "limits_u64": rdst_amd.select_segments_limits("uint64")}
    if args.out and os.path.exists(args.out):                              # the two parts may be measured in two runs
        with open(args.out) as f:
            old = json.load(f)
        summary.update({key: old[key] for key in ("stream_max_sweep", "crossing", "table", "slower_than_sort_baseline", "slower_than_loop_baseline")
                        if key in old})
    if args.device_offsets:
        rows = device_offsets(torch, rdst_amd, args)
        summary = {key: summary[key] for key in ("tool", "device", "reps", "limits_u32", "limits_u64")}
        summary["device_offsets"] = rows
        for mode in ("async", "wait"):                                      # by the unrounded medians
            summary[f"slower_than_baseline_{mode}"] = [[r["shape"], r["keys"], r["index"], r["ranks"], r[f"baseline_over_{mode}"]] for r in rows
                                                       if r["baseline_copy_sync_host_entry"]["ms"] < r[mode]["ms"]]
    elif args.stream_max_sweep:
        summary["stream_max_sweep"] = stream_max_sweep(torch, rdst_amd, args)
        summary["crossing"] = {}
        for kind in ("u32", "u64"):
            for set_name in ("median", "deciles"):
                rows = [r for r in summary["stream_max_sweep"] if r["keys"] == kind and r["ranks"] == set_name]
                wins = [r["n"] for r in rows if r["far_over_stream"] >= 1.0]
                loses = [r["n"] for r in rows if r["far_over_stream"] < 1.0]
                summary["crossing"][f"{kind}_{set_name}"] = {"longest_n_stream_wins": max(wins) if wins else None,
                                                            "shortest_n_far_wins": min(loses) if loses else None}
    else:
        summary["table"] = table(torch, rdst_amd, args)
    if "table" in summary:
        summary["slower_than_sort_baseline"], summary["slower_than_loop_baseline"] = slower_lists(summary["table"])
    print(json.dumps({key: v for key, v in summary.items() if key not in ("stream_max_sweep", "table", "device_offsets")}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
