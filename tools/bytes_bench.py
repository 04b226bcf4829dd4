"""Device-entry timings of [u8; N] sorts (rdst_hip_sort_bytes_device), one JSON line per case and a summary object.

    python tools/bytes_bench.py [--reps 5] [--scale 1.0] [--out profiles/bytes_bench.json]

Every case sorts a fresh copy of the same input (the copy is not timed), after one untimed warm-up sort; the time is
HIP events on the tensor's stream around the entry point, median over --reps.  The [u8; 16] case takes the widened
integer route the entry keeps for N <= 16; "pairs_u64_u32" is the stable pair sort the N > 16 route is built on, alone,
for reference.  --scale shrinks every size (smoke runs).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import rdst_amd
    from rdst_amd import _lib
    torch.cuda.set_device(0)
    lib = _lib.load()
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
    summary = {"tool": "tools/bytes_bench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "results": results}
    print(json.dumps(summary))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
