"""The key sample may be wrong; the sort may not ("The flags only steer; every route still proves its own
preconditions exactly, so a wrong guess costs time, never correctness").

From 2^26 keys up presample_kernel reads 8 192 keys at the positions k * (n / 8192) and leaves six words in the plan.  The
positions are a closed formula, so the inputs here are CONSTRUCTED around them (tests/helpers.py; tests/test_sample_helpers.py
holds the builders to their names): the sample is shown one thing and the other keys are another, each flag is told both ways
one hit below and at its threshold, and pass A's own per-key checks are visited at pass A's borders.  Every sort is checked
three ways: the output equals torch.sort of the mapped keys element for element; the six words the device's sample left
(rdst_amd.last_sample) equal their numpy restatement (helpers.sample_verdict) — which is what shows that the lie was told; and
the route is the one the restated rules give (helpers.predicted_route) wherever they determine it.

What cannot be reached here: the 8-byte prediction's `hits >= 16` edge binds only from 4.3 x 10^9 keys up (est > 2 x tile with
16 hits), so only its `est` edge is placed (2 x tile against 2 x tile + 1); under split_always (mode 17) the most recent plan
is the last part's, so the sample words are recorded, not asserted, there."""
import numpy as np
import pytest

import helpers as H
from test_gpu_lengths import _mapped, geometry

pytestmark = pytest.mark.gpu

N0 = (1 << 26) + 12_345                      # the sample is alive, n / 8192 truncates
N4_SHIPPED, N8_SHIPPED = 3 * (1 << 26) + 16_897, 100_000_003   # past the shipped thresholds of 4- and 8-byte keys
N_SMALL = 3_000_001                          # no sample: pass A's borders once more, cheaply
SEED = 0x5D570400
WIDTH = {"uint32": 32, "int32": 32, "float32": 32, "uint64": 64, "int64": 64, "float64": 64}
ROUTES = {}                                  # group -> route -> sorts (printed by the last test)


@pytest.fixture(autouse=True)
def _restore(gpu):
    yield
    gpu.set_hybrid(True, 0)
    gpu.set_tuning()


class Runner:
    """sorts mapped-space inputs under one route setting and collects every disagreement (all reported at the end of the test)"""

    def __init__(self, torch, gpu, group, mode=1, min_len=1):
        self.torch, self.gpu, self.group = torch, gpu, group
        self.mode, self.tuning = mode, H.route_tuning(mode, min_len)
        self.bad, self.sorts = [], 0
        gpu.set_hybrid(mode, min_len)

    def gen(self, salt):
        return self.torch.Generator(device="cuda").manual_seed(SEED + salt)

    def sort(self, m, name, what, atomic_ok=None, want_route=None, not_route=None, want_depth=None, check_sample=True, sorted_want=None):
        """m: mapped keys as int bits.  Returns (route, sample)."""
        torch, gpu = self.torch, self.gpu
        n, w, kind = m.numel(), WIDTH[name], np.dtype(name).kind
        src = H.unmapped_bits(torch, m, name)
        keys = src.clone()
        gpu.sort_device_tensor(keys.view(getattr(torch, name)))
        route, sample = gpu.last_route(), gpu.last_sample()
        self.sorts += 1
        tally = ROUTES.setdefault(self.group, {})
        tally[route] = tally.get(route, 0) + 1
        tag = (self.group, what, name, n, f"mode {self.mode}", route, sample)
        sampled = src[H.sample_index(torch, n, "cuda")].cpu().numpy().view(name)
        verdict = H.sample_verdict(sampled, self.tuning, n=n)
        if check_sample and sample != verdict:
            self.bad.append(("sample words differ from their restatement", verdict) + tag)
        if want_depth is not None and verdict["win_shift"] != want_depth:
            self.bad.append((f"the builder promised window depth {want_depth}", verdict) + tag)
        s_src = _mapped(torch, src, kind)
        want = torch.sort(s_src).values if sorted_want is None else sorted_want
        got = _mapped(torch, keys, kind)
        if not bool(torch.equal(want, got)):
            first = int(torch.nonzero(want != got)[0])
            self.bad.append(("OUTPUT DIFFERS", f"first at {first}", geometry(n, w // 8)) + tag)
        # the route the restated rules give
        stray = bool((H.top_bits(m, w, verdict["win_shift"]) != verdict["win_top"]).any()) if verdict["win_shift"] else False
        if stray:
            atomic_ok = False
        counts = torch.bincount(H.top_bits(m, w, 16), minlength=65536)
        rule = H.predicted_route(verdict, n, w // 8, self.tuning, atomic_ok, int((counts >= H.GIANT_MIN).sum()), int(counts.max()))
        if self.tuning["split_always"]:
            rule = None                                   # the slice goes in parts: the last part's route
        for expect, why in ((rule, "restated rules"), (want_route, "the case")):
            if expect is not None and route != expect:
                self.bad.append((f"route: {why} say {expect}", f"stray={stray} atomic_ok={atomic_ok}") + tag)
        if not_route is not None and route == not_route:
            self.bad.append((f"route must not be {not_route}",) + tag)
        del src, keys, s_src, want, got, counts
        return route, sample

    def done(self):
        self.gpu.device_status()
        print(f"group {self.group} mode {self.mode}: {self.sorts} sorts, routes so far {ROUTES.get(self.group)}")
        assert not self.bad, f"{len(self.bad)} of {self.sorts} sorts disagree:\n" + "\n".join(map(str, self.bad[:12]))


def test_no_sample_no_words(gpu):
    """a sort too short for a pipeline, one too short for a sample, and one on the LSD-only setting: six zeros"""
    import torch
    zeros = dict.fromkeys(H.SAMPLE_WORDS, 0)
    for n, mode in ((1000, 1), (N_SMALL, 1), (N0, 0)):
        r = Runner(torch, gpu, "0", mode=mode)
        _route, sample = r.sort(H.rand_mapped(torch, n, 32, r.gen(n % 97), "cuda"), "uint32", f"n={n}")
        assert sample == zeros
        r.done()


# ---- A: the window at every depth, every type --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(WIDTH))
def test_a_window_depth(gpu, name):
    import torch
    r = Runner(torch, gpu, "A")
    w = WIDTH[name]
    for d in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16):
        for pat in ("zeros", "ones", "mixed") if d else ("zeros",):
            m = H.window_keys(torch, N0, w, d, H.window_pattern(pat, d), r.gen(d * 8 + len(pat)), "cuda")
            # up to a byte shared the buckets below it are uniform: the atomic route takes the sort.  More than a byte: the
            # window stops at 8 bits and the buckets' own top bits are shared (the sample or the areas find out): the rules say
            r.sort(m, name, f"shared {d} {pat}", atomic_ok=True if d <= 8 else None, want_route="atomic" if d <= 8 else None,
                   want_depth=min(d, 8))
    m = H.window_keys(torch, N4_SHIPPED if w == 32 else N8_SHIPPED, w, 5, H.window_pattern("mixed", 5), r.gen(99), "cuda")
    r2 = Runner(torch, gpu, "A", mode=1, min_len=0)          # the shipped setting
    r2.sort(m, name, "shared 5 mixed, shipped", atomic_ok=True, want_route="atomic", want_depth=5)
    r2.bad += r.bad
    r2.done()


# ---- B: the sample lies about the window -------------------------------------------------------------------------------

def _strays(torch, r, name, n, depths, salt):
    w = WIDTH[name]
    for d in depths:
        pat = H.window_pattern("mixed", d)
        base = H.window_keys(torch, n, w, d, pat, r.gen(salt + d), "cuda")
        for pos in H.stray_positions(n, w // 8):
            for flip in sorted({1, 1 << (d - 1)}):            # the lowest shared bit, the top bit
                m = base.clone()
                m[pos:pos + 1] = H.set_top(m[pos:pos + 1], w, d, pat ^ flip)
                r.sort(m, name, f"depth {d} stray {pos} ^{flip}", not_route="atomic", want_depth=d)
                del m
        del base


@pytest.mark.parametrize("name,mode", [("uint32", 1), ("float32", 1), ("int64", 1), ("uint32", 10), ("uint64", 8)])
def test_b_one_key_outside_the_window(gpu, name, mode):
    import torch
    r = Runner(torch, gpu, "B", mode=mode)
    _strays(torch, r, name, N0, (1, 4, 8) if mode == 1 else (4,), 100)
    r.done()


@pytest.mark.parametrize("name", ["uint32", "uint64"])
def test_b_one_key_outside_the_window_shipped_setting(gpu, name):
    import torch
    r = Runner(torch, gpu, "B", mode=1, min_len=0)
    _strays(torch, r, name, N4_SHIPPED if name == "uint32" else N8_SHIPPED, (4,), 150)
    r.done()


@pytest.mark.parametrize("name,mode", [("uint32", 1), ("int32", 10), ("float64", 1), ("uint64", 8)])
def test_b_window_in_the_sample_only(gpu, name, mode):
    import torch
    r = Runner(torch, gpu, "B", mode=mode)
    w = WIDTH[name]
    for d in (1, 4, 8):                                        # (ii) strays in every tile: only the sampled keys share d bits
        pat = H.window_pattern("mixed", d)
        sampled = H.window_keys(torch, N0, w, d, pat, r.gen(200 + d), "cuda")[H.sample_index(torch, N0, "cuda")]
        m = H.with_sample(torch, H.rand_mapped(torch, N0, w, r.gen(210 + d), "cuda"), sampled)
        r.sort(m, name, f"sample shares {d}, the rest nothing", not_route="atomic", want_depth=d)
    # (iii) guessed too deep: the sample shares 8 bits, the population 3
    pat8 = H.window_pattern("mixed", 8)
    sampled = H.window_keys(torch, N0, w, 8, pat8, r.gen(220), "cuda")[H.sample_index(torch, N0, "cuda")]
    m = H.with_sample(torch, H.window_keys(torch, N0, w, 3, pat8 >> 5, r.gen(221), "cuda"), sampled)
    r.sort(m, name, "sample shares 8, population 3", not_route="atomic", want_depth=8)
    # ... and too shallow: the population shares 8 bits but for two sampled keys that leave the sample only 3 — the buckets
    # are then 32 times over-full (the sample's top bytes show it, or the areas and slots find out): atomic or not, exact
    m = H.window_keys(torch, N0, w, 8, pat8, r.gen(222), "cuda")
    pos = H.sample_index(torch, N0, "cuda")[5:7]
    two = torch.tensor([(pat8 >> 5 << 5) | 0b00000, (pat8 >> 5 << 5) | 0b11111], device="cuda", dtype=m.dtype)
    H.plant(m, pos, H.set_top(m[pos], w, 8, two))
    r.sort(m, name, "population shares 8, sample 3", want_depth=3)
    r.done()


# ---- C: each flag, told both ways, at its threshold --------------------------------------------------------------------

def _limit(n, kb):
    return 12 + 4 * H.LOCAL_TILE[kb] * H.PRESAMPLE_KEYS // n


def _one_prefix(torch, m, w, prefix):
    return H.set_top(m, w, 16, prefix)


def _third_on_a_byte(torch, m, w, byte=0x47):
    third = torch.arange(m.numel(), device=m.device) % 3 == 0
    m[third] = H.set_top(m[third], w, 8, byte)
    return m


def _flag_cases(torch, r, name, n, flags):
    """(what, mapped keys, atomic_ok) for the flags asked for, built one at a time"""
    w, kb = WIDTH[name], WIDTH[name] // 8
    uniform = lambda salt: H.rand_mapped(torch, n, w, r.gen(salt), "cuda")                      # noqa: E731
    if "gross" in flags:
        lim = _limit(n, kb)
        for hits in (lim - 1, lim):
            s = H.gross_sample(torch, w, hits, r.gen(300 + hits), "cuda")
            yield f"gross {hits}/{lim}, population uniform", H.with_sample(torch, uniform(301), s), True
            heavy = uniform(302)
            share = torch.arange(n, device="cuda") % H.PRESAMPLE_KEYS < hits                    # the sample's share of the keys, for real
            heavy[share] = _one_prefix(torch, heavy[share], w, 0xF008)
            yield f"gross {hits}/{lim}, population has the bucket", H.with_sample(torch, heavy, s), False
        s = H.spread_sample(torch, w, r.gen(303), "cuda")
        yield "gross: clean sample, every other key on one prefix", H.with_sample(torch, _one_prefix(torch, uniform(304), w, 0x4711), s), False
    if "top" in flags:
        for hits in (63, 64):
            s = H.top_sample(torch, w, hits, r.gen(310 + hits), "cuda")
            yield f"top {hits}/64, population uniform", H.with_sample(torch, uniform(311), s), True
        s = H.spread_sample(torch, w, r.gen(312), "cuda")
        yield "top: clean sample, a third of the keys on one top byte", H.with_sample(torch, _third_on_a_byte(torch, uniform(313), w), s), False
        s = H.top_sample(torch, w, 64, r.gen(314), "cuda")
        yield "top 64/64, a third of the keys on that top byte", H.with_sample(torch, _third_on_a_byte(torch, uniform(315), w), s), False
    if "dups" in flags:
        few = lambda m: (m & H._signed(0xFFFF0000, 32)) | ((m & 15) * 4099)                     # noqa: E731  low halves of 16 values
        for dups in (4999, 5000):
            s = H.dups_sample(torch, dups, r.gen(320 + dups % 7), "cuda")
            yield f"dups {dups}/5000, population's low halves uniform", H.with_sample(torch, uniform(321), s), True
            yield f"dups {dups}/5000, population's low halves take 16 values", H.with_sample(torch, few(uniform(322)), s), True
        s = H.spread_sample(torch, w, r.gen(323), "cuda")
        yield "dups: clean sample, population's low halves take 16 values", H.with_sample(torch, few(uniform(324)), s), True
    if "predict8" in flags:
        for hits in (1023, 1024) if n == N0 else (1000,):
            s = H.bytes_sample(torch, w, 1, hits, r.gen(330 + hits % 5), "cuda")
            yield f"predict {hits} hits, population uniform", H.with_sample(torch, uniform(331), s), True
            yield f"predict {hits} hits, population has the byte", H.with_sample(torch, H.bytes_population(torch, uniform(332), w, 1, hits), s), False
    if "predict4" in flags:
        for nbytes, hits in ((24, 320), (25, 320)) if n > N0 else ((1, 2559), (1, 2560)):
            s = H.bytes_sample(torch, w, nbytes, hits, r.gen(340 + nbytes + hits % 3), "cuda")
            yield f"predict {nbytes} bytes x {hits}, population uniform", H.with_sample(torch, uniform(341), s), True
            yield f"predict {nbytes} bytes x {hits}, population has them", H.with_sample(torch, H.bytes_population(torch, uniform(342), w, nbytes, hits), s), False


@pytest.mark.parametrize("name,mode,flags", [
    ("uint32", 1, ("gross", "top", "dups", "predict4")), ("float32", 1, ("gross", "top", "dups")), ("int32", 10, ("gross", "top")),
    ("uint32", 11, ("gross", "top", "dups", "predict4")), ("uint32", 12, ("gross", "top", "dups")), ("uint32", 14, ("gross", "top", "predict4")),
    ("uint64", 1, ("gross", "top", "predict8")), ("float64", 1, ("gross", "top", "predict8")), ("int64", 8, ("gross", "top", "predict8")),
    ("uint64", 12, ("gross", "top", "predict8")), ("uint64", 14, ("gross", "top", "predict8"))])
def test_c_flags_at_their_thresholds(gpu, name, mode, flags):
    import torch
    r = Runner(torch, gpu, "C", mode=mode)
    seen = {k: set() for k in H.SAMPLE_WORDS}
    for what, m, atomic_ok in _flag_cases(torch, r, name, N0, flags):
        _route, sample = r.sort(m, name, what, atomic_ok=atomic_ok, want_depth=0)
        for k in seen:
            seen[k].add(sample[k])
        del m
    r.done()
    told = {"gross": "gross_skew", "top": "top_skew", "dups": "low_dups"}
    for f in flags:                                            # both sides of every threshold were really told
        if f in told:
            assert seen[told[f]] == {0, 1}, (f, seen)
    if ("predict4" in flags and mode == 11) or ("predict8" in flags and mode != 14):
        assert seen["predict_lsd"] == {0, 1}, seen            # (4-byte keys at this length: one byte cannot outvote 4 096 tables)


def test_c_predict_4_byte_keys_24_and_25_giant_sized_bytes(gpu):
    """25 top bytes of 320 hits need est >= 1.25 x 65 536 from 320 hits: 2^29 keys"""
    import torch
    n = (1 << 29) + 12_345
    seen = set()
    for mode in (1, 14):
        r = Runner(torch, gpu, "C", mode=mode)
        for what, m, atomic_ok in _flag_cases(torch, r, "uint32", n, ("predict4",)):
            _route, sample = r.sort(m, "uint32", what, atomic_ok=atomic_ok, want_depth=0)
            if mode == 1:
                seen.add(sample["predict_lsd"])
            del m
        r.done()
    assert seen == {0, 1}


def test_c_predict_8_byte_keys_est_at_twice_the_tile(gpu):
    """1 000 hits of 8 192 on one top byte: est = n x 1000 / 2^21 is 32 768 = 2 x tile at 68 721 573 keys (no prediction) and
    32 769 at one key more"""
    import torch
    seen = []
    for n in (68_721_573, 68_721_574):
        assert n * 1000 // (H.PRESAMPLE_KEYS * 256) == 2 * H.LOCAL_TILE[8] + (n & 1 ^ 1) and n % H.PRESAMPLE_KEYS
        r = Runner(torch, gpu, "C")
        for what, m, atomic_ok in _flag_cases(torch, r, "uint64", n, ("predict8",)):
            _route, sample = r.sort(m, "uint64", what, atomic_ok=atomic_ok, want_depth=0)
            seen.append(sample["predict_lsd"])
            del m
        r.done()
    assert seen == [0, 0, 1, 1]


@pytest.mark.parametrize("name", ["uint32", "uint64"])
def test_c_flags_on_the_shipped_setting(gpu, name):
    import torch
    r = Runner(torch, gpu, "C", mode=1, min_len=0)
    for what, m, atomic_ok in _flag_cases(torch, r, name, N4_SHIPPED if name == "uint32" else N8_SHIPPED, ("gross", "top")):
        r.sort(m, name, what, atomic_ok=atomic_ok, want_depth=0)
        del m
    r.done()


# ---- D: modes that must not change results -----------------------------------------------------------------------------

def _bag(torch, r):
    """a mixed bag from A-C, both widths: (name, what, mapped keys)"""
    for name in ("uint32", "float32", "uint64", "int64"):
        w = WIDTH[name]
        salt = 400 + w + len(name)
        yield name, "window 5", H.window_keys(torch, N0, w, 5, H.window_pattern("mixed", 5), r.gen(salt), "cuda")
        base = H.window_keys(torch, N0, w, 4, H.window_pattern("ones", 4), r.gen(salt + 1), "cuda")
        base[N0 - 1:] = H.set_top(base[N0 - 1:], w, 4, 0b0111)
        yield name, "window 4, last key outside", base
        cases = list(_flag_cases(torch, r, name, N0, ("top",)))
        yield name, cases[2][0], cases[2][1]
        del cases


@pytest.mark.parametrize("mode", [1, 5, 7, 12, 14, 15, 16, 17])
def test_d_modes_that_must_not_change_results(gpu, mode):
    import torch
    r = Runner(torch, gpu, "D", mode=mode)
    for name, what, m in _bag(torch, r):
        if mode == 15 and WIDTH[name] == 32:
            continue                                           # (the second form of the 8-byte K4)
        _route, sample = r.sort(m, name, what, check_sample=mode != 17)
        if mode == 5:
            assert sample == dict.fromkeys(H.SAMPLE_WORDS, 0), sample
        del m
    r.done()


# ---- E: nearly degenerate slices with the sample alive -----------------------------------------------------------------

EQUAL = {"uint32": 0x47474747, "float32": 0xFFC00001,          # (mapped 0xFFC00001: the NaN 0x7FC00001)
         "uint64": 0x4747474747474747, "int64": 0xC747474747474747}


@pytest.mark.parametrize("name", list(EQUAL))
@pytest.mark.parametrize("mode", [1, 10, 11, 14])
def test_e_all_keys_equal_but_one(gpu, name, mode):
    import torch
    r = Runner(torch, gpu, "E", mode=mode)
    w = WIDTH[name]
    it = torch.int32 if w == 32 else torch.int64
    eq = H._signed(EQUAL[name], w)
    base = torch.full((N0,), eq, dtype=it, device="cuda")
    if name == "float32":
        assert np.isnan(H.unmapped_bits(torch, base[:1], name).view(torch.float32).item())
    route, _s = r.sort(base, name, "all equal", sorted_want=_mapped(torch, H.unmapped_bits(torch, base, name), np.dtype(name).kind))
    for pos in (0, H.not_sampled(N0, [N0 // 2 + 3])[0], N0 - 1):
        for delta in (-1, 1):
            m = base.clone()
            m[pos] = eq + delta
            r.sort(m, name, f"one key {delta:+d} at {pos}")
            del m
    # two values, sorted, and with a single inversion at their border
    half = N0 // 2 + 11
    m = base.clone()
    m[half:] = eq + 1
    r.sort(m, name, "two values, sorted", sorted_want=_mapped(torch, H.unmapped_bits(torch, m, name), np.dtype(name).kind))
    m[half - 1], m[half] = eq + 1, eq
    r.sort(m, name, "two values, one inversion")
    r.done()


# ---- F: pass A's own per-key checks at pass A's borders ----------------------------------------------------------------

def _swaps(torch, r, name, base, what, atomic_ok):
    w, n = WIDTH[name], base.numel()
    kind = np.dtype(name).kind
    sorted_image = _mapped(torch, H.unmapped_bits(torch, base, name), kind)
    assert bool((sorted_image[1:] > sorted_image[:-1]).all()), "the builder promised strictly increasing keys"
    want_route = "atomic" if atomic_ok else None
    r.sort(base, name, f"{what}, untouched", atomic_ok=atomic_ok, want_route=want_route, sorted_want=sorted_image)
    skipped = 0
    for i in H.swap_spots(n, w // 8):
        m = base.clone()
        a, b = m[i].clone(), m[i + 1].clone()
        if bool(a == b):
            skipped += 1
            continue
        m[i], m[i + 1] = b, a
        r.sort(m, name, f"{what}, swapped at {i}", atomic_ok=atomic_ok, want_route=want_route, sorted_want=sorted_image)
        del m
    assert skipped == 0


@pytest.mark.parametrize("name", ["uint32", "float32", "uint64"])
@pytest.mark.parametrize("n", [N0, N_SMALL])
def test_f_swapped_neighbours_at_pass_a_borders(gpu, name, n):
    import torch
    r = Runner(torch, gpu, "F")
    w = WIDTH[name]
    _swaps(torch, r, name, H.increasing_keys(torch, n, w, r.gen(500), "cuda"), "uniform", True)
    # ids below a quarter of the range: with the sample alive the window drops by two bits.  Whether the atomic route then
    # keeps the sort is the areas' arithmetic, not the window's: sorted keys reach a top digit's eight areas as whole tiles in
    # turn (16.5 tiles of 4-byte keys per digit here: one area gets three, over its room; 8-byte keys: four each, inside
    # it), so the route is recorded and the restated rules judge what follows a refusal
    _swaps(torch, r, name, H.increasing_keys(torch, n, w, r.gen(501), "cuda", below_bits=w - 2), "below a quarter of the range", None)
    if name == "uint32":     # 2^26 consecutive ids: the sample sees 128 top bytes of the window, 64 hits each
        _swaps(torch, r, name, H.increasing_keys(torch, n, w, None, "cuda", dense_from=0x2000_0000), "dense ids", None)
    r.done()


def test_zz_routes_reported(gpu):
    """(not a check of the library) prints which routes each group's sorts ended on; B, C and E must have reached the fallbacks
    and A must have stayed on the atomic route wherever a byte or less was shared"""
    print("routes per group:", ROUTES)
    if all(g in ROUTES for g in "ABCE"):                       # (a run of the whole file)
        assert set(ROUTES["B"]) - {"atomic"} and set(ROUTES["C"]) >= {"atomic", "hybrid", "lsd"} and set(ROUTES["E"]) - {"atomic"}
        assert ROUTES["A"].get("atomic", 0) >= 6 * 25
