"""Device-entry timings of the key-value sort whose length lives in device memory (rdst_hip_sort_pairs_device_devlen) against
the known-length entry (rdst_hip_sort_pairs_device), one JSON line per case and a summary object.

    python tools/devlen_bench.py [--reps 5] [--scale 1.0] [--out profiles/devlen_bench.json]

(u32, u32) and (u64, u32) pairs at a capacity of 10^8, with the length m in {capacity, capacity / 2, capacity / 16, 10^5, 0}.
The device-length entry sorts the first m of `capacity` pairs, m read from a device buffer; the yardstick sorts a slice of
len = m (m = 0: an empty stream interval, two events back to back).  Both run in the same process, alternating, each from
a fresh copy of the same input (the copy is not timed), after one untimed warm-up round; the time is HIP events on the
stream around the entry point, median over --reps, all of them kept.  At m = capacity the two results are compared; one
more run of each under rdst_hip_set_profiling gives every case's stage times.  At small m the device-length time is the floor
of capacity-sized launches that return early (K3's one block per tile of the capacity, per level).  --scale shrinks the
capacity (smoke runs)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_alternating(torch, fns, reps):
    """`fns`: name -> fn(prep); fn(None) prepares (untimed), fn(True) is timed.  One warm-up round, then `reps` rounds, each
    running every fn once"""
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
    """one more run of fn under rdst_hip_set_profiling: the stage times of its pipeline summed by name"""
    rdst_amd.set_profiling(True)
    try:
        prep = fn(None)
        torch.cuda.synchronize()
        fn(prep)
        torch.cuda.synchronize()
        by = {}
        for r in range(rdst_amd.profile_runs()):
            got = rdst_amd.profile_run(r, 0)
            for name, _level, ms in (got["stages"] if got else ()):
                by[name] = round(by.get(name, 0.0) + ms, 4)
        return by
    finally:
        rdst_amd.set_profiling(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import rdst_amd
    torch.cuda.set_device(0)
    cap = int(1e8 * args.scale)
    lengths = [cap, cap // 2, cap // 16, min(cap, 100_000), 0]
    results = []
    for kname, kdtype in (("u32", torch.int32), ("u64", torch.int64)):
        g = torch.Generator(device="cuda")
        g.manual_seed(8 * kdtype.itemsize)
        info = torch.iinfo(kdtype)
        # signed storage (every torch kernel takes it), sorted through unsigned views of the same memory
        src_k = torch.randint(info.min, info.max, (cap,), dtype=kdtype, device="cuda", generator=g)
        src_v = torch.arange(cap, dtype=torch.int32, device="cuda")
        store_k, store_v = torch.empty_like(src_k), torch.empty_like(src_v)
        udtype = torch.uint32 if kdtype == torch.int32 else torch.uint64
        keys_src, keys, vals = src_k.view(udtype), store_k.view(udtype), store_v.view(torch.uint32)
        tk, tv = torch.empty_like(store_k).view(udtype), torch.empty_like(store_v).view(torch.uint32)
        length = torch.zeros(1, dtype=torch.int64, device="cuda")
        for m in lengths:
            def devlen(prep, m=m):
                if prep is None:
                    store_k.copy_(src_k)
                    store_v.copy_(src_v)
                    length.fill_(m)
                    return True
                rdst_amd.sort_pairs_device_devlen_tensor(keys, vals, length, tk, tv, check=False)
                return None

            def known(prep, m=m):
                if prep is None:
                    store_k.copy_(src_k)
                    store_v.copy_(src_v)
                    return True
                if m:                                       # (m = 0: nothing between the two events)
                    rdst_amd.sort_pairs_device_tensor(keys[:m], vals[:m], tk, tv, check=False)
                return None

            fns = {"devlen": devlen, "known_length": known}
            ms = _time_alternating(torch, fns, args.reps)
            rdst_amd.device_status()
            med = {k: v[len(v) // 2] for k, v in ms.items()}
            rec = {"case": f"pairs_{kname}_u32", "capacity": cap, "m": m, "devlen_ms": round(med["devlen"], 4),
                   "known_length_ms": round(med["known_length"], 4),
                   "devlen_over_known": round(med["devlen"] / med["known_length"], 3) if m and med["known_length"] > 0 else None,
                   "devlen_spread": round(ms["devlen"][-1] / ms["devlen"][0], 3) if ms["devlen"][0] > 0 else None,
                   "known_length_spread": round(ms["known_length"][-1] / ms["known_length"][0], 3) if m and ms["known_length"][0] > 0 else None,
                   "devlen_ms_all": [round(x, 4) for x in ms["devlen"]], "known_length_ms_all": [round(x, 4) for x in ms["known_length"]]}
            if m == cap:
                # (the last timed run was the yardstick's: its result is in keys / vals)
                want_k, want_v = keys.clone(), vals.clone()
                devlen(devlen(None))
                rdst_amd.device_status()
                assert torch.equal(want_k.view(torch.uint8), keys.view(torch.uint8)) and torch.equal(want_v.view(torch.uint8), vals.view(torch.uint8)), \
                    "the two entries disagree"
                head = keys[:3].view(torch.uint8).cpu().numpy().view(f"<u{kdtype.itemsize}").tolist()
                assert head == sorted(head)
                del want_k, want_v
                rec["results_equal"] = True
            elif m:
                # the prefix is sorted, the pair behind it is the input's
                devlen(devlen(None))
                rdst_amd.device_status()
                edge = keys[m - 2:m].view(torch.uint8).cpu().numpy().view(f"<u{kdtype.itemsize}").tolist()
                assert edge == sorted(edge) and torch.equal(keys[m:m + 4].view(torch.uint8), keys_src[m:m + 4].view(torch.uint8))
            rec["devlen_stages_ms"] = _profiled(torch, rdst_amd, devlen)
            rec["known_length_stages_ms"] = _profiled(torch, rdst_amd, known) if m else {}
            rdst_amd.device_status()
            print(json.dumps(rec), flush=True)
            results.append(rec)
        del src_k, src_v, store_k, store_v, keys_src, keys, vals, tk, tv
        torch.cuda.empty_cache()
    # the floor: what the capacity's launches cost when next to nothing is sorted — every pass running (the shortest m > 0)
    # and every pass skipped (m = 0)
    small = min(m for m in lengths if m)
    floors = {r["case"]: {"passes_run_ms": r["devlen_ms"], "m": small} for r in results if r["m"] == small}
    for r in results:
        if r["m"] == 0:
            floors[r["case"]]["all_skipped_ms"] = r["devlen_ms"]
    summary = {"tool": "tools/devlen_bench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "capacity": cap,
               "early_return_floor_ms": floors, "results": results}
    print(json.dumps({k: v for k, v in summary.items() if k != "results"}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
