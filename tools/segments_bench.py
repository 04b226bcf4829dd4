"""Development aid: the segmented sort (rdst_hip_sort_segments_device / _pairs_device) against a loop of the slice entry
(rdst_hip_sort_device / rdst_hip_sort_pairs_device) over the same segments — the only way to sort many slices before the
segmented entries existed.  Both are timed on the host clock from the first call to the end of the stream (the loop is
launch-bound: its cost is the host's), five repeats each on fresh copies of the same input; the loop calls the C entry
through ctypes with precomputed pointers.  Writes profiles/segments_bench.json: median and spread (min, max) per shape
and type, and the three conditions DESIGN.md §2f reports:
  all-long shape: the segmented entry's median lies within the loop's own run-to-run spread (it runs the same launches);
  every shape with at least 1 024 batched segments: the segmented entry is faster than the loop;
  every shape with at least 1 024 batched segments: the device-offsets entry (rdst_hip_sort_segments_device_offsets, the
  table already in device memory, its scratch allocated once) has its median within the host-offsets entry's run-to-run
  spread or below it — both measured in the same run.
With --nowait the tool measures one more condition instead, again both sides in the same run, median of five and spread:
the nowait entries (rdst_hip_sort_segments_device_offsets_nowait: long segments on the device's tiled route) against the
tmp_elems > 0 mode of rdst_hip_sort_segments_device_offsets (a stream wait, then one whole-slice pipeline per long segment) on
4 096 x 65 536, 2^14 log-normal lengths of median 10^4, 64 x 2^20 and 1 x 2^26, and writes profiles/segments_nowait_bench.json.
  the first two shapes (thousands of long segments of a few tiles): the nowait median lies below the tmp mode's median by
  more than the two spreads (max - min) together; the last two: the ratio only.
usage: python tools/segments_bench.py [--quick] [--nowait] [--out profiles/segments_bench.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rdst_amd
from rdst_amd import _lib
from rdst_amd.radix_sort import key_info

REPEATS = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shapes(quick):
    rng = np.random.default_rng(0x5E6)
    lognormal = np.maximum(0, np.exp(rng.normal(np.log(500.0), 1.0, size=1 << 14))).astype(np.int64)
    out = [("2^16 x 16", np.full(1 << 16, 16, dtype=np.int64)),
           ("2^14 x 1024", np.full(1 << 14, 1024, dtype=np.int64)),
           ("2^12 x 16384", np.full(1 << 12, 16384, dtype=np.int64)),
           ("2^14 log-normal (median 500)", lognormal),
           ("64 x 2^24", np.full(64, 1 << 24, dtype=np.int64))]
    if quick:
        out = [(name, l[:max(4, len(l) // 64)]) for name, l in out]
    return out


def timed(fn, restore):
    times = []
    for _ in range(REPEATS):
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        rdst_amd.device_status()
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "all_ms": times}


def run(name, lengths, kdtype, vdtype):
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    n = int(off[-1])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    it = {4: torch.int32, 8: torch.int64}[torch.empty(0, dtype=kdtype).element_size()]
    info = torch.iinfo(it)
    src = torch.randint(info.min, info.max, (n,), dtype=it, device="cuda", generator=gen).view(kdtype)
    keys = torch.empty_like(src)
    vals = base = None
    vb = 0
    if vdtype is not None:
        base = torch.arange(n, dtype=torch.int32, device="cuda").view(vdtype)
        vals = torch.empty_like(base)
        vb = base.element_size()
    kind, kb, levels = key_info(kdtype)
    _items, counts, need = rdst_amd.segments_plan(off, n, kdtype, vb)
    longest = int(lengths.max())
    tmp = torch.empty(longest, dtype=kdtype, device="cuda")          # scratch for the loop's longest slice and for the long class
    tmpv = torch.empty(longest, dtype=vdtype, device="cuda") if vdtype is not None else None
    lib = _lib.load()
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    kp, tp = keys.data_ptr(), vp(tmp.data_ptr())
    starts = [int(x) for x in off[:-1]]
    lens = [int(x) for x in lengths]

    def restore():
        keys.copy_(src)
        if vals is not None:
            vals.copy_(base)

    def new():
        rdst_amd.sort_segments_device_tensor(keys, off, tmp=tmp, values=vals, tmp_values=tmpv, check=False)

    dev_off = torch.from_numpy(off.astype(np.int64)).cuda()
    scratch = torch.empty(rdst_amd.segments_device_offsets_scratch_bytes(len(lengths)), dtype=torch.uint8, device="cuda")
    has_long = counts[2] != 0      # without long segments: the fully asynchronous mode (no tmp)

    def dev():
        rdst_amd.sort_segments_device_offsets_tensor(keys, dev_off, tmp=tmp if has_long else None, values=vals,
                                                     tmp_values=tmpv if has_long else None, scratch=scratch, check=False)

    if vdtype is None:
        def loop():
            f = lib.rdst_hip_sort_device
            for s, l in zip(starts, lens):
                rc = f(vp(kp + s * kb), tp, l, kb, kind, levels, stream)
                if rc:
                    _lib.check(rc)
    else:
        vptr, tvp = vals.data_ptr(), vp(tmpv.data_ptr())

        def loop():
            f = lib.rdst_hip_sort_pairs_device
            for s, l in zip(starts, lens):
                rc = f(vp(kp + s * kb), vp(vptr + s * vb), tp, tvp, l, kb, kind, levels, vb, stream)
                if rc:
                    _lib.check(rc)

    r_new = timed(new, restore)
    got = keys.clone()
    r_dev = timed(dev, restore)
    assert torch.equal(got.view(it), keys.view(it)), "the host-offsets and the device-offsets entry disagree"
    r_loop = timed(loop, restore)
    assert torch.equal(got.view(it), keys.view(it)), "the segmented entry and the loop disagree"
    batched = counts[0] + counts[1]
    row = {"shape": name, "keys": str(kdtype).replace("torch.", ""), "values": str(vdtype).replace("torch.", "") if vdtype is not None else None,
           "segments": int(len(lengths)), "n": n, "class_counts": list(counts), "segmented": r_new, "device_offsets": r_dev,
           "device_offsets_mode": "tmp" if has_long else "asynchronous", "loop": r_loop, "speedup_median": r_loop["median_ms"] / r_new["median_ms"]}
    if counts[2] == len(lengths):      # all long: the same launches as the loop
        row["within_loop_spread"] = bool(r_loop["min_ms"] <= r_new["median_ms"] <= r_loop["max_ms"])
    if batched >= 1024:
        row["faster_than_loop"] = bool(r_new["median_ms"] < r_loop["median_ms"])
        row["device_offsets_within_host_spread_or_below"] = bool(r_dev["median_ms"] <= r_new["max_ms"])
    print(f"{name:30s} {row['keys']:7s} {str(row['values']):7s} n={n:.2e} classes={counts}: segmented {r_new['median_ms']:9.3f} ms "
          f"[{r_new['min_ms']:.3f}, {r_new['max_ms']:.3f}]  device offsets {r_dev['median_ms']:9.3f} ms [{r_dev['min_ms']:.3f}, {r_dev['max_ms']:.3f}]  loop {r_loop['median_ms']:9.3f} ms [{r_loop['min_ms']:.3f}, {r_loop['max_ms']:.3f}]  "
          f"x{row['speedup_median']:.1f}", flush=True)
    return row


def nowait_shapes(quick):
    rng = np.random.default_rng(0x5E7)
    lognormal = np.maximum(0, np.exp(rng.normal(np.log(1.0e4), 1.0, size=1 << 14))).astype(np.int64)
    out = [("4096 x 65536", np.full(4096, 65536, dtype=np.int64), True),
           ("2^14 log-normal (median 10^4)", lognormal, True),
           ("64 x 2^20", np.full(64, 1 << 20, dtype=np.int64), False),
           ("1 x 2^26", np.full(1, 1 << 26, dtype=np.int64), False)]
    if quick:
        out = [(name, l[:max(1, len(l) // 64)] if len(l) > 64 else l // 64, cond) for name, l, cond in out]
    return out


def run_nowait(name, lengths, conditioned, kdtype, vdtype):
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    n = int(off[-1])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    it = {4: torch.int32, 8: torch.int64}[torch.empty(0, dtype=kdtype).element_size()]
    info = torch.iinfo(it)
    src = torch.randint(info.min, info.max, (n,), dtype=it, device="cuda", generator=gen).view(kdtype)
    keys = torch.empty_like(src)
    vals = base = tmpv = None
    vb = 0
    if vdtype is not None:
        base = torch.arange(n, dtype=torch.int32, device="cuda").view(vdtype)
        vals, tmpv = torch.empty_like(base), torch.empty_like(base)
        vb = base.element_size()
    _items, counts, _need = rdst_amd.segments_plan(off, n, kdtype, vb)
    tmp = torch.empty_like(src)                                         # len elements: what the nowait entries ask for (the tmp mode needs the longest)
    dev_off = torch.from_numpy(off.astype(np.int64)).cuda()
    scratch = torch.empty(rdst_amd.segments_nowait_scratch_bytes(len(lengths), n, kdtype, vb), dtype=torch.uint8, device="cuda")

    def restore():
        keys.copy_(src)
        if vals is not None:
            vals.copy_(base)

    def tmp_mode():
        rdst_amd.sort_segments_device_offsets_tensor(keys, dev_off, tmp=tmp, values=vals, tmp_values=tmpv, scratch=scratch, check=False)

    def nowait():
        rdst_amd.sort_segments_device_offsets_nowait_tensor(keys, dev_off, tmp=tmp, values=vals, tmp_values=tmpv, scratch=scratch, check=False)

    r_tmp = timed(tmp_mode, restore)
    got = keys.clone()
    gotv = vals.clone() if vals is not None else None
    r_now = timed(nowait, restore)
    assert torch.equal(got.view(it), keys.view(it)), "the tmp mode and the nowait entry disagree"
    assert vals is None or torch.equal(gotv.view(torch.int32), vals.view(torch.int32)), "the tmp mode and the nowait entry disagree on the values"
    spreads = (r_now["max_ms"] - r_now["min_ms"]) + (r_tmp["max_ms"] - r_tmp["min_ms"])
    row = {"shape": name, "keys": str(kdtype).replace("torch.", ""), "values": str(vdtype).replace("torch.", "") if vdtype is not None else None,
           "segments": int(len(lengths)), "n": n, "class_counts": list(counts), "scratch_bytes": int(scratch.numel()), "tmp_mode": r_tmp, "nowait": r_now,
           "nowait_over_tmp_mode_median": r_now["median_ms"] / r_tmp["median_ms"], "spreads_together_ms": spreads}
    if conditioned:
        row["nowait_below_tmp_mode_by_more_than_the_spreads"] = bool(r_tmp["median_ms"] - r_now["median_ms"] > spreads)
    print(f"{name:30s} {row['keys']:7s} {str(row['values']):7s} n={n:.2e} classes={counts}: tmp mode {r_tmp['median_ms']:9.3f} ms "
          f"[{r_tmp['min_ms']:.3f}, {r_tmp['max_ms']:.3f}]  nowait {r_now['median_ms']:9.3f} ms [{r_now['min_ms']:.3f}, {r_now['max_ms']:.3f}]  "
          f"nowait / tmp mode {row['nowait_over_tmp_mode_median']:.3f}", flush=True)
    return row


def main_nowait(args):
    rows = []
    for name, lengths, conditioned in nowait_shapes(args.quick):
        for kdtype, vdtype in ((torch.uint32, None), (torch.uint64, None), (torch.uint32, torch.uint32)):
            rows.append(run_nowait(name, lengths, conditioned, kdtype, vdtype))
            torch.cuda.empty_cache()
    key = "nowait_below_tmp_mode_by_more_than_the_spreads"
    result = {"tool": "tools/segments_bench.py --nowait", "repeats": REPEATS, "quick": args.quick, "device": torch.cuda.get_device_name(0), "rows": rows,
              key: all(r[key] for r in rows if key in r)}
    out = args.out or os.path.join(ROOT, "profiles", "segments_nowait_bench.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"shapes with thousands of long segments: nowait below the tmp mode by more than the two spreads together: {result[key]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a 64th of every shape's segments (a check of the tool itself)")
    ap.add_argument("--nowait", action="store_true", help="the nowait entries against the tmp mode instead (profiles/segments_nowait_bench.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.nowait:
        return main_nowait(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "segments_bench.json")
    rows = []
    for name, lengths in shapes(args.quick):
        for kdtype, vdtype in ((torch.uint32, None), (torch.uint64, None), (torch.uint32, torch.uint32)):
            rows.append(run(name, lengths, kdtype, vdtype))
            torch.cuda.empty_cache()
    result = {"tool": "tools/segments_bench.py", "repeats": REPEATS, "quick": args.quick, "device": torch.cuda.get_device_name(0), "rows": rows,
              "all_long_within_loop_spread": all(r["within_loop_spread"] for r in rows if "within_loop_spread" in r),
              "batched_faster_than_loop": all(r["faster_than_loop"] for r in rows if "faster_than_loop" in r),
              "device_offsets_within_host_spread_or_below": all(r["device_offsets_within_host_spread_or_below"] for r in rows
                                                                if "device_offsets_within_host_spread_or_below" in r)}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"all-long within the loop's spread: {result['all_long_within_loop_spread']}; batched shapes faster than the loop: "
          f"{result['batched_faster_than_loop']}; device offsets within the host-offsets spread or below: "
          f"{result['device_offsets_within_host_spread_or_below']}")


if __name__ == "__main__":
    main()
