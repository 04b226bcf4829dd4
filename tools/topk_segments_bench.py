"""Device timings of the segmented partial sort (rdst_hip_topk_segments_device) against the two ways the library offered the
same result before it, and — for information only — torch.topk(dim=1).  One JSON line per case and a summary object.

    python tools/topk_segments_bench.py [--reps 5] [--only sweep|table] [--scale 1.0] [--out profiles/topk_segments_bench.json]
    python tools/topk_segments_bench.py --device-offsets [--reps 7] [--scale 1.0] [--out profiles/topk_segments_offsets_bench.json]

sweep   one segment per call, lengths 2^17 .. 2^23, u32 and u64 keys, k = 64: the stream class forced against the far class
        forced, both through rdst_hip_set_topk_segments_stream_max.  The crossing is where the library's default belongs.
table   rows x row length 65 536 x 64, 4 096 x 4 096, 1 024 x 16 384, 64 x 131 072, 8 x 2^20 and a ragged table with lengths
        from 1 to 2^18; k = 1, 8, 64, 1 024; u32, f32 and u64 keys only, u32 and f32 with an int32 index.  Baselines:
          loop    topk_device_tensor per row.  At most --loop-rows rows are timed and the time is scaled to the table: the
                  cost is a per-call floor, row after row (loop_rows_timed says how many ran);
          sort    a copy of the array, the segmented sort of the copy (with an index: the segmented pair sort against a
                  per-row iota), a gather of k per row.
        Tables with rows beyond the default stream_max also run with the stream class forced for them (stream_forced_ms, for
        information: the default comes from the sweep's one segment per call).
        One more run under rdst_hip_set_profiling gives the time of each class's launch, and for the stream class the bytes
        it streams per second and per workgroup (every read of every level counted, from the select restated on the host
        for a sample of rows).

--device-offsets   the table's shapes and one row of 2^24 keys, with the borders in DEVICE memory
        (rdst_hip_topk_segments_device_offsets); k = 1, 64, 1 024; u32 and u64 keys only, f32 with an int32 index:
          async      far_capacity = 0: the plan and three counted launches, nothing comes to the host;
          wait       far_capacity = len: the plan, one wait for the stream, the host entry's classes;
          today      what a caller with device offsets pays without the entry: the table copied to the host, a synchronise,
                     rdst_hip_topk_segments_device;
          host       rdst_hip_topk_segments_device with a table that is on the host already: the plan's bare cost is what
                     async and wait add to it.
        All four give the same bits (checked).

The candidates run in one process, alternating, after one untimed warm-up round; the time is HIP events on the stream around
the calls, median over --reps with all of them kept.  Every result is compared with the sort baseline's."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def _class_ms(torch, rdst_amd, fn):
    """ms of the wave-, block- and stream-class launches (stage 13, the class in bits 8..15) and of everything the far class
    enqueued, from one profiled run"""
    from rdst_amd import _lib
    lib = _lib.load()
    rdst_amd.set_profiling(True)
    try:
        fn()
        torch.cuda.synchronize()
        out = {"wave": 0.0, "block": 0.0, "stream": 0.0, "far": 0.0}
        for r in range(rdst_amd.profile_runs()):
            buf, kinds = (ctypes.c_float * 64)(), (ctypes.c_uint32 * 64)()
            n, nk = ctypes.c_uint32(0), ctypes.c_uint32(0)
            _lib.check(lib.rdst_hip_profile_run(r, buf, 64, ctypes.byref(n)))
            _lib.check(lib.rdst_hip_profile_run_stages(r, kinds, 64, ctypes.byref(nk)))
            for i in range(min(n.value, nk.value)):
                code, cls = kinds[i] & 0xFF, (kinds[i] >> 8) & 0xFF
                out[("wave", "block", "stream")[cls] if code == _lib.RDST_STAGE_SEGMENTS and cls < 3 else "far"] += float(buf[i])
        return {name: round(ms, 4) for name, ms in out.items()}
    finally:
        rdst_amd.set_profiling(False)


def _keys(torch, kind, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    if kind == "f32":
        return torch.randn(n, dtype=torch.float32, device="cuda", generator=g)
    if kind == "u64":
        return torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=g).view(torch.uint64)
    return torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=g).view(torch.uint32)


def sweep(torch, rdst_amd, args):
    results = []
    for kind in ("u32", "u64"):
        for e in range(17, 24):
            n, k = 1 << e, 64
            keys = _keys(torch, kind, n, e)
            off = np.array([0, n], dtype=np.uint64)
            rdst_amd.set_topk_segments_stream_max(1)
            scratch = torch.empty(rdst_amd.topk_segments_scratch_bytes(1, n, k, keys.dtype), dtype=torch.uint8, device="cuda")
            out = {}

            def run(border, name):
                rdst_amd.set_topk_segments_stream_max(border)
                out[name] = rdst_amd.topk_segments_device_tensor(keys, off, k, scratch=scratch, check=False)[0]

            ms = _time_alternating(torch, {"stream": lambda: run(1 << 24, "stream"), "far": lambda: run(1, "far")}, args.reps)
            rdst_amd.device_status()
            assert torch.equal(out["stream"].view(torch.uint8), out["far"].view(torch.uint8)), "stream and far class disagree"
            rec = {"part": "sweep", "keys": kind, "n": n, "k": k, "stream": _stats(ms["stream"]), "far": _stats(ms["far"]),
                   "far_over_stream": round(ms["far"][len(ms["far"]) // 2] / ms["stream"][len(ms["stream"]) // 2], 3)}
            print(json.dumps(rec), flush=True)
            results.append(rec)
    rdst_amd.set_topk_segments_stream_max(0)
    return results


def _tables(scale):
    rng = np.random.default_rng(5)
    for rows, cols in ((65536, 64), (4096, 4096), (1024, 16384), (64, 131072), (8, 1 << 20)):
        rows = max(1, int(rows * scale))
        yield f"{rows}x{cols}", np.arange(rows + 1, dtype=np.uint64) * np.uint64(cols), cols
    lengths = np.unique(np.concatenate([[1, 1 << 18], (2.0 ** rng.uniform(0, 18, size=max(2, int(400 * scale)))).astype(np.int64)]))
    yield "ragged_1_to_2^18", np.concatenate([[0], np.cumsum(rng.permutation(lengths))]).astype(np.uint64), None


def _reads(keys_host, off, k, tile, rows=8):
    """reads of a stream-class segment: its select levels + the collection, from the select restated on the host for the
    first `rows` stream-class rows; (mean reads, rows looked at)"""
    import topk_segments_inputs as S
    got = []
    for lo, hi in zip(off[:-1], off[1:]):
        if int(hi - lo) > tile and len(got) < rows:
            got.append(S.stream_depth(keys_host[int(lo):int(hi)], min(k, int(hi - lo)), False, tile)[0] + 1)
    return (round(float(np.mean(got)), 2), len(got)) if got else (None, 0)


def table(torch, rdst_amd, args):
    results = []
    np_dtype = {"u32": np.uint32, "f32": np.float32, "u64": np.uint64}
    for shape, off, cols in _tables(args.scale):
        n, n_seg = int(off[-1]), len(off) - 1
        lens = (off[1:] - off[:-1]).astype(np.int64)
        for kind, indexed in (("u32", False), ("f32", False), ("u64", False), ("u32", True), ("f32", True)):
            keys = _keys(torch, kind, n, n_seg % 11 + len(kind))
            ib = 4 if indexed else 0
            index = torch.int32 if indexed else None
            wm, bm, sm, _ksm = rdst_amd.topk_segments_limits(keys.dtype, ib)
            copy = torch.empty_like(keys)
            longest = int(lens.max())
            tmp = torch.empty(longest, dtype=keys.dtype, device="cuda") if longest > bm else None
            iota_src = vals = tmp_vals = None
            if indexed:
                starts = torch.from_numpy(np.repeat(off[:-1].astype(np.int64), lens)).cuda()
                iota_src = (torch.arange(n, dtype=torch.int64, device="cuda") - starts).to(torch.int32)   # the per-row iota, made once
                vals = torch.empty_like(iota_src)
                tmp_vals = torch.empty(longest, dtype=torch.int32, device="cuda") if longest > bm else None
                del starts
            signed = keys if keys.dtype.is_floating_point else keys.view(torch.int32 if keys.element_size() == 4 else torch.int64)
            keys_host = None
            for k in (1, 8, 64, 1024):
                k_s = np.minimum(lens, k)
                # where row s, slot j lives in the sorted copy (j < k_s), for the gather
                rows_at = torch.from_numpy(np.repeat(np.arange(n_seg, dtype=np.int64), k_s)).cuda()
                slot_at = torch.from_numpy(np.concatenate([np.arange(x, dtype=np.int64) for x in k_s]) if cols is None else
                                           np.tile(np.arange(min(k, cols), dtype=np.int64), n_seg)).cuda()
                src_at = torch.from_numpy(off[:-1].astype(np.int64)).cuda()[rows_at] + slot_at
                scratch = torch.empty(rdst_amd.topk_segments_scratch_bytes(n_seg, longest, k, keys.dtype, ib), dtype=torch.uint8, device="cuda")
                out_k = torch.zeros((n_seg, k), dtype=keys.dtype, device="cuda")
                out_i = torch.zeros((n_seg, k), dtype=torch.int32, device="cuda") if indexed else None
                base_k, base_i = torch.zeros_like(out_k), (torch.zeros_like(out_i) if indexed else None)
                loop_rows = min(n_seg, args.loop_rows)
                loop_scratch = torch.empty(max(rdst_amd.topk_scratch_bytes(longest, min(k, longest), keys.dtype, ib), 256), dtype=torch.uint8, device="cuda")

                def segments():
                    rdst_amd.topk_segments_device_tensor(keys, off, k, index=index, scratch=scratch, check=False, out=(out_k, out_i))

                def loop():
                    for s in range(loop_rows):
                        rdst_amd.topk_device_tensor(keys[int(off[s]):int(off[s + 1])], int(k_s[s]), index=index, scratch=loop_scratch, check=False)

                def sort():
                    copy.copy_(keys)
                    if indexed:
                        vals.copy_(iota_src)
                        rdst_amd.sort_segments_device_tensor(copy, off, tmp=tmp, values=vals, tmp_values=tmp_vals, check=False)
                        base_i[rows_at, slot_at] = vals[src_at]
                    else:
                        rdst_amd.sort_segments_device_tensor(copy, off, tmp=tmp, check=False)
                    base_k.view(torch.uint8).view(signed.dtype)[rows_at, slot_at] = copy.view(signed.dtype)[src_at]

                def stream_forced():                        # for information: the rows beyond the default border on one workgroup each
                    rdst_amd.set_topk_segments_stream_max(1 << 24)
                    try:
                        segments()
                    finally:
                        rdst_amd.set_topk_segments_stream_max(0)

                fns = {"segments": segments, "loop": loop, "sort": sort}
                if longest > sm and k <= bm:
                    fns["stream_forced"] = stream_forced
                if cols is not None and not args.no_torch:
                    fns["torch_topk"] = lambda: torch.topk(signed.view(n_seg, cols), min(k, cols), dim=1, largest=False, sorted=True)
                ms = _time_alternating(torch, fns, args.reps)
                rdst_amd.device_status()
                assert torch.equal(out_k.view(torch.uint8), base_k.view(torch.uint8)), "the segmented partial sort and the sort baseline disagree"
                if indexed:
                    assert torch.equal(out_i, base_i), "the positions disagree"
                med = {name: v[len(v) // 2] for name, v in ms.items()}
                loop_ms = med["loop"] * n_seg / loop_rows
                _items, counts, _far = rdst_amd.topk_segments_plan(off, n, k, keys.dtype, ib)
                classes = _class_ms(torch, rdst_amd, segments)
                rec = {"part": "table", "shape": shape, "segments": n_seg, "n": n, "keys": kind, "index": ib, "k": k, "class_counts": list(counts),
                       "segments_call": _stats(ms["segments"]), "sort_baseline": _stats(ms["sort"]),
                       "loop_baseline_ms": round(loop_ms, 3), "loop_rows_timed": loop_rows, "loop_spread": round(ms["loop"][-1] / ms["loop"][0], 3),
                       "torch_topk_ms": round(med["torch_topk"], 4) if "torch_topk" in med else None,
                       "stream_forced_ms": round(med["stream_forced"], 4) if "stream_forced" in med else None,
                       "sort_over_segments": round(med["sort"] / med["segments"], 2), "loop_over_segments": round(loop_ms / med["segments"], 2),
                       "class_ms": classes, "results_equal": True}
                if counts[2]:
                    if keys_host is None:
                        keys_host = keys.view(signed.dtype).cpu().numpy().view(np_dtype[kind])
                    reads, looked = _reads(keys_host, off, k, bm)
                    stream_bytes = int(lens[(lens > bm) & (lens <= sm)].sum()) * keys.element_size()
                    rec["stream_reads_per_segment"] = reads
                    rec["stream_reads_rows_restated"] = looked
                    if classes["stream"] > 0 and reads:
                        # the launch's time is the longest segments' when there are fewer workgroups than compute units; with
                        # more it is the table's bytes over the launch: both are given
                        rec["stream_gb_per_s_launch"] = round(stream_bytes * reads / classes["stream"] / 1e6, 1)
                        rec["stream_gb_per_s_per_workgroup"] = round(stream_bytes * reads / classes["stream"] / 1e6 / min(counts[2], args.cus), 2)
                print(json.dumps(rec), flush=True)
                results.append(rec)
                del scratch, out_k, out_i, base_k, base_i, rows_at, slot_at, src_at, loop_scratch
            del keys, copy, tmp, iota_src, vals, tmp_vals, signed
            torch.cuda.empty_cache()
    return results


def device_offsets(torch, rdst_amd, args):
    results = []
    tables = list(_tables(args.scale)) + [("1x2^24", np.array([0, 1 << 24], dtype=np.uint64), 1 << 24)]
    for shape, off, _cols in tables:
        n, n_seg = int(off[-1]), len(off) - 1
        longest = int((off[1:] - off[:-1]).max())
        toff = torch.from_numpy(off.astype(np.int64)).cuda()
        for kind, indexed in (("u32", False), ("u64", False), ("f32", True)):
            keys = _keys(torch, kind, n, n_seg % 11 + len(kind))
            ib = 4 if indexed else 0
            index = torch.int32 if indexed else None
            _wm, bm, sm, _ksm = rdst_amd.topk_segments_limits(keys.dtype, ib)
            for k in (1, 64, 1024):
                outs = {name: (torch.zeros((n_seg, k), dtype=keys.dtype, device="cuda"), torch.zeros((n_seg, k), dtype=torch.int32, device="cuda") if indexed else None)
                        for name in ("async", "wait", "today", "host")}
                s_async = torch.empty(rdst_amd.topk_segments_device_offsets_scratch_bytes(n_seg, 0, k, keys.dtype, ib), dtype=torch.uint8, device="cuda")
                s_wait = torch.empty(rdst_amd.topk_segments_device_offsets_scratch_bytes(n_seg, n, k, keys.dtype, ib), dtype=torch.uint8, device="cuda")
                s_host = torch.empty(rdst_amd.topk_segments_scratch_bytes(n_seg, longest, k, keys.dtype, ib), dtype=torch.uint8, device="cuda")

                def run_async():
                    rdst_amd.topk_segments_device_offsets_tensor(keys, toff, k, index=index, scratch=s_async, check=False, out=outs["async"])

                def run_wait():
                    rdst_amd.topk_segments_device_offsets_tensor(keys, toff, k, index=index, scratch=s_wait, far_capacity=n, check=False, out=outs["wait"])

                def run_today():
                    table = toff.cpu().numpy().astype(np.uint64)            # the copy waits for the stream
                    rdst_amd.topk_segments_device_tensor(keys, table, k, index=index, scratch=s_host, check=False, out=outs["today"])

                def run_host():
                    rdst_amd.topk_segments_device_tensor(keys, off, k, index=index, scratch=s_host, check=False, out=outs["host"])

                ms = _time_alternating(torch, {"async": run_async, "wait": run_wait, "today": run_today, "host": run_host}, args.reps)
                rdst_amd.device_status()
                for name in ("async", "wait", "today"):
                    assert torch.equal(outs[name][0].view(torch.uint8), outs["host"][0].view(torch.uint8)), f"{name} and the host entry disagree"
                    assert not indexed or torch.equal(outs[name][1], outs["host"][1]), f"{name}: the positions disagree"
                med = {name: v[len(v) // 2] for name, v in ms.items()}
                rec = {"part": "device_offsets", "shape": shape, "segments": n_seg, "n": n, "keys": kind, "index": ib, "k": k,
                       "class_counts_async": list(rdst_amd.topk_segments_plan_device(toff, n, k, keys.dtype, ib, unbounded_stream=True)[1]),
                       "class_counts_wait": list(rdst_amd.topk_segments_plan(off, n, k, keys.dtype, ib)[1]),
                       "async": _stats(ms["async"]), "wait": _stats(ms["wait"]), "today": _stats(ms["today"]), "host": _stats(ms["host"]),
                       "today_over_async": round(med["today"] / med["async"], 2), "today_over_wait": round(med["today"] / med["wait"], 2),
                       "async_minus_host_ms": round(med["async"] - med["host"], 4), "wait_minus_host_ms": round(med["wait"] - med["host"], 4),
                       "results_equal": True}
                print(json.dumps(rec), flush=True)
                results.append(rec)
                del outs, s_async, s_wait, s_host
            del keys
            torch.cuda.empty_cache()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the row counts of the table")
    ap.add_argument("--only", choices=("sweep", "table"), default=None)
    ap.add_argument("--loop-rows", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch.topk column out")
    ap.add_argument("--device-offsets", action="store_true", help="the entry with the borders in device memory against copy + synchronise + host entry")
    args = ap.parse_args()
    import torch
    import rdst_amd
    torch.cuda.set_device(0)
    args.cus = torch.cuda.get_device_properties(0).multi_processor_count
    summary = {"tool": "tools/topk_segments_bench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "compute_units": args.cus,
               "limits_u32": rdst_amd.topk_segments_limits("uint32"), "limits_u64": rdst_amd.topk_segments_limits("uint64")}
    if args.device_offsets:
        summary["device_offsets"] = device_offsets(torch, rdst_amd, args)
        for name in ("async", "wait"):
            summary[f"{name}_slower_than_today"] = [[r["shape"], r["keys"], r["index"], r["k"], r[f"today_over_{name}"]] for r in summary["device_offsets"]
                                                    if r[f"today_over_{name}"] < 1.0]
        print(json.dumps({key: v for key, v in summary.items() if key != "device_offsets"}))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(summary, f, indent=1)
        return
    if args.out and os.path.exists(args.out):                              # the two parts may be measured in two runs
        with open(args.out) as f:
            old = json.load(f)
        summary.update({key: old[key] for key in ("sweep", "crossing", "table", "slower_than_sort_baseline", "slower_than_loop_baseline") if key in old})
    if args.only in (None, "sweep"):
        summary["sweep"] = sweep(torch, rdst_amd, args)
        summary["crossing"] = {}
        for kind in ("u32", "u64"):
            wins = [r["n"] for r in summary["sweep"] if r["keys"] == kind and r["far_over_stream"] >= 1.0]
            loses = [r["n"] for r in summary["sweep"] if r["keys"] == kind and r["far_over_stream"] < 1.0]
            summary["crossing"][kind] = {"longest_n_stream_wins": max(wins) if wins else None, "shortest_n_far_wins": min(loses) if loses else None}
    if args.only in (None, "table"):
        summary["table"] = table(torch, rdst_amd, args)
        summary["slower_than_sort_baseline"] = [[r["shape"], r["keys"], r["index"], r["k"]] for r in summary["table"] if r["sort_over_segments"] < 1.0]
        summary["slower_than_loop_baseline"] = [[r["shape"], r["keys"], r["index"], r["k"]] for r in summary["table"] if r["loop_over_segments"] < 1.0]
    print(json.dumps({key: v for key, v in summary.items() if key not in ("sweep", "table")}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
