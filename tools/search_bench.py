"""Device timings of the binary search (rdst_hip_search_device) beside the floor of the bytes it must move and beside
torch.searchsorted.  One JSON line per case and a summary object.

    python tools/search_bench.py [--reps 7] [--repeats 1] [--scale 1.0] [--out profiles/search_bench.json] [--ab LIB_A LIB_B [--ab-rounds 4]]

Inputs: a sorted haystack of m = 2^16, 2^24, 2^28 keys (u32, u64, f32; u128 up to 2^24) and 2^26 needles (--scale shrinks both),
the needles uniformly random, the same sorted, and random within 1 % of the key range.  Integer keys stay below the sign bit
and the floats are finite, so that torch's order by value and the library's order by mapped bits agree and the results can be
compared.  Per input, in one process, alternating after an untimed warm-up round, HIP events on the stream around each call,
median over --reps with every time kept:
  search      the call, side="left", 8-byte positions (what torch.searchsorted returns)
  both        the call with both outputs
  torch       torch.searchsorted on the same tensors and the synchronise it ends in (no 16-byte keys)
  copy        rdst_hip_stream_copy of half the bytes `search` must move — the needles read and the positions written, and for the
              sorted needles the haystack once — i.e. the same traffic: the floor
--repeats runs the whole list that many times and keeps every repeat's medians: the spread of torch's own medians is the margin
inside which "equal to torch" is said.  --ab runs bench.py's headline in child processes on two builds of the library,
alternating, and records both series."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.runs_bench import _ab, _median, _time_alternating  # noqa: E402

KEYS = (("u32", 4, 1 << 28), ("u64", 8, 1 << 28), ("f32", 4, 1 << 28), ("u128", 16, 1 << 24))   # (name, bytes, largest haystack)
HAYSTACKS = (1 << 16, 1 << 24, 1 << 28)
NEEDLES = 1 << 26
SHAPES = ("random", "sorted", "one_percent")


def _random_keys(torch, rdst_amd, key, n, gen, lo=0.0, hi=1.0):
    """n keys of `key`, uniform over the fraction [lo, hi) of the range the bench uses"""
    if key == "f32":
        return ((torch.rand(n, device="cuda", generator=gen) * (hi - lo) + lo) * 2e6 - 1e6).to(torch.float32)
    if key == "u32":
        span = 1 << 31
        return torch.randint(int(lo * span), int(hi * span), (n,), device="cuda", generator=gen, dtype=torch.int64).to(torch.int32).view(torch.uint32)
    span = 1 << 62
    high = torch.randint(int(lo * span), int(hi * span), (n,), device="cuda", generator=gen, dtype=torch.int64)
    if key == "u64":
        return high.view(torch.uint64)
    low = torch.randint(0, 1 << 62, (n,), device="cuda", generator=gen, dtype=torch.int64)
    return torch.stack([low, high], dim=1).contiguous()


def _for_torch(torch, key, t):
    return t if key == "f32" else t.view(torch.int32 if key == "u32" else torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=1)
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
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)
    nn = max(4096, int(NEEDLES * args.scale))
    cases = []
    for repeat in range(0 if args.only_ab else args.repeats):
        for key, kb, largest in KEYS:
            wide = key if key == "u128" else None
            name = {"u32": "uint32", "u64": "uint64", "f32": "float32"}.get(key, key)
            for m in HAYSTACKS:
                if m > largest:
                    continue
                m = max(1024, int(m * args.scale))
                hay = _random_keys(torch, rdst_amd, key, m, gen)
                rdst_amd.sort_device_tensor(hay, key=wide)
                scratch = torch.empty(rdst_amd.search_scratch_bytes(m, nn, name), dtype=torch.uint8, device="cuda")
                lower, upper = torch.empty(nn, dtype=torch.int64, device="cuda"), torch.empty(nn, dtype=torch.int64, device="cuda")
                for shape in SHAPES:
                    needles = _random_keys(torch, rdst_amd, key, nn, gen, *((0.495, 0.505) if shape == "one_percent" else (0.0, 1.0)))
                    if shape == "sorted":
                        rdst_amd.sort_device_tensor(needles, key=wide)
                    moved = nn * kb + nn * 8 + (m * kb if shape == "sorted" else 0)
                    half = moved // 2 // 16 * 16
                    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
                    fns = {"search": lambda: rdst_amd.search_device_tensor(hay, needles, side="left", scratch=scratch, check=False, key=wide, out=lower),
                           "both": lambda: rdst_amd.search_device_tensor(hay, needles, side="both", scratch=scratch, check=False, key=wide, out=(lower, upper)),
                           "copy": lambda: _lib.check(lib.rdst_hip_stream_copy(dst.data_ptr(), src.data_ptr(), half, stream))}
                    if not wide:
                        t_hay, t_needles = _for_torch(torch, key, hay), _for_torch(torch, key, needles)

                        def torch_way():
                            out = torch.searchsorted(t_hay, t_needles)
                            torch.cuda.synchronize()
                            return out
                        fns["torch"] = torch_way
                    ms = _time_alternating(torch, fns, args.reps)
                    rdst_amd.device_status()
                    rdst_amd.search_device_tensor(hay, needles, side="left", scratch=scratch, key=wide, out=lower)
                    state = rdst_amd.search_state(scratch)
                    if not wide:
                        assert torch.equal(lower, torch_way()), (key, m, shape)
                    med = {k: _median(v) for k, v in ms.items()}
                    case = {"repeat": repeat, "key": key, "m": m, "needles": nn, "shape": shape, "bytes_moved": moved, "tiles_staged": state["staged"],
                            "tiles_table": state["table"], "ms": ms, "median_ms": med, "copy_over_search": med["copy"] / med["search"],
                            "gneedles_per_s": nn / med["search"] / 1e6}
                    if "torch" in med:
                        case["torch_over_search"] = med["torch"] / med["search"]
                    print(json.dumps(case), flush=True)
                    cases.append(case)
                    del needles, src, dst, fns
                    torch.cuda.empty_cache()
                del hay, scratch, lower, upper
                torch.cuda.empty_cache()
    summary = {"tool": "tools/search_bench.py", "reps": args.reps, "repeats": args.repeats, "scale": args.scale, "cases": cases}
    if args.ab:
        summary["bench_ab"] = {"unit": "Gkeys/s (bench.py --gpus 1 --steps 6 --warmup 2)", "series": _ab(args.ab, args.ab_rounds, 6, 2)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    print(json.dumps({k: v for k, v in summary.items() if k != "cases"}))


if __name__ == "__main__":
    main()
