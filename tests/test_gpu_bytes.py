"""[u8; N] keys wider than 16 bytes on the device (src/radix_key_impl.rs:78-85: rows sort lexicographically): the host
entry, the device entry, the Python builder on a HIP tensor, a non-default stream, an unaligned row base, every round
boundary of the refinement, runs of duplicates on both sides of the comparison kernel's limits, records keyed by a byte
string, and one full-size slice.  Expected orders come from numpy: np.sort on V<N> (unsigned lexicographic) and the
stable np.lexsort for records."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = (17, 20, 24, 31, 32, 33, 40, 64, 100, 255, 256, 1000, 4096)
SIZES = (0, 1, 2, 3, 257, 100_003)
SMALL = 256  # longest run the comparison kernel takes (rdst_bytes.hip, BYTES_SMALL)


def _rows(rng, n, N):
    a = rng.integers(0, 256, size=(n, N), dtype=np.uint8)
    a[rng.random((n, N)) < 0.3] = 0  # ties on leading bytes, as in test_byte_array_keys
    return a


def _expected(a):
    n, N = a.shape
    if n == 0:
        return a.copy()
    return np.sort(a.view(f"V{N}").ravel()).view(np.uint8).reshape(n, N)


def _routes(gpu, a):
    """(name, sorted copy) for every way in: host entry, device entry, builder on a HIP tensor, a side stream, a row base
    one byte past an allocation's start."""
    import torch
    n, N = a.shape
    out = []
    got = a.copy()
    gpu.sort_host_array(got, key="bytes")
    out.append(("host", got))
    t = torch.from_numpy(a.copy()).cuda()
    gpu.sort_bytes_device_tensor(t)
    out.append(("device", t.cpu().numpy()))
    t = torch.from_numpy(a.copy()).cuda()
    gpu.radix_sort_unstable(t, key="bytes")
    out.append(("builder", t.cpu().numpy()))
    t = torch.from_numpy(a.copy()).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gpu.radix_sort_builder(t, key="bytes").sort()
    s.synchronize()
    out.append(("stream", t.cpu().numpy()))
    buf = torch.zeros(n * N + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = torch.from_numpy(a.ravel().copy()).cuda()
    v = buf[1:].view(n, N)
    assert v.data_ptr() % 2 == 1 or n == 0
    gpu.radix_sort_unstable(v, key="bytes")
    out.append(("offset", v.cpu().numpy()))
    assert int(buf[0]) == 0
    return out


def _check_all(gpu, a, what):
    exp = _expected(a)
    for name, got in _routes(gpu, a):
        assert np.array_equal(got, exp), (what, name)


@pytest.mark.parametrize("N", WIDTHS)
def test_random_rows_every_entry(gpu, N):
    rng = np.random.default_rng(0xB17E + N)
    for n in SIZES:
        _check_all(gpu, _rows(rng, n, N), (N, n))


@pytest.mark.parametrize("N", (17, 20, 24, 33, 64, 256))
def test_common_prefix_reaches_every_round(gpu, N):
    """P shared bytes then random suffixes: the prefix sort leaves one run, and the rounds end at every boundary (inside
    the first word, on it, past it, in the zero-padded last chunk)."""
    rng = np.random.default_rng(0x9F + N)
    for P in sorted({7, 8, 9, 15, 16, N - 5, N - 1}):
        if not 0 < P < N:
            continue
        a = _rows(rng, 30_000, N)
        a[:, :P] = rng.integers(0, 256, size=P, dtype=np.uint8)
        a[1::5] = a[0::5][: a[1::5].shape[0]]  # some exact duplicates
        _check_all(gpu, a, (N, P))


@pytest.mark.parametrize("N", (24, 64, 1000, 4096))
def test_runs_of_duplicates(gpu, N):
    """Runs of identical rows of length 2, SMALL - 1, SMALL, SMALL + 1 (both sides of the comparison kernel's limit; at
    N = 1000 and 4096 most of them cannot be staged and take the radix rounds), shuffled among distinct rows."""
    rng = np.random.default_rng(0xD0 + N)
    parts = []
    for length in (2, SMALL - 1, SMALL, SMALL + 1):
        for _ in range(3):
            base = _rows(rng, 1, N)
            base[0, :8] = 7  # one shared prefix for every run: the runs separate in the rounds
            parts.append(np.repeat(base, length, axis=0))
    parts.append(_rows(rng, 5_000, N))
    a = np.concatenate(parts)
    a = a[rng.permutation(a.shape[0])]
    _check_all(gpu, a, N)


@pytest.mark.parametrize("N", (20, 64, 4096))
def test_a_hundred_thousand_identical_rows(gpu, N):
    import torch
    rng = np.random.default_rng(N)
    a = np.repeat(_rows(rng, 1, N), 100_000, axis=0)
    a = np.concatenate([a, _rows(rng, 1_000, N)])
    a = a[rng.permutation(a.shape[0])]
    exp = _expected(a)
    got = a.copy()
    gpu.sort_host_array(got, key="bytes")
    assert np.array_equal(got, exp)
    t = torch.from_numpy(a.copy()).cuda()
    gpu.radix_sort_unstable(t, key="bytes")
    assert np.array_equal(t.cpu().numpy(), exp)


@pytest.mark.parametrize("N", (17, 40, 256, 2048))
def test_zipf_run_sizes(gpu, N):
    rng = np.random.default_rng(0x21F + N)
    distinct = _rows(rng, 4_000, N)
    distinct[:, : N // 2] = 0  # long shared prefixes: the runs reach the later rounds
    pick = np.minimum(rng.zipf(1.3, size=120_000), distinct.shape[0]) - 1
    a = distinct[pick]
    exp = _expected(a)
    got = a.copy()
    gpu.sort_host_array(got, key="bytes")
    assert np.array_equal(got, exp)
    import torch
    t = torch.from_numpy(a.copy()).cuda()
    gpu.sort_bytes_device_tensor(t)
    assert np.array_equal(t.cpu().numpy(), exp)


def _record_dtype(N, form):
    key = {"u1": ("u1", (N,)), "S": f"S{N}", "V": f"V{N}"}[form]
    # odd offset, odd row size: no alignment anywhere
    return np.dtype({"names": ["tag", "k", "seq"], "formats": ["u1", key, "<u4"], "offsets": [0, 1, 1 + N], "itemsize": N + 6})


@pytest.mark.parametrize("N", (1, 3, 8, 20, 32, 77))
@pytest.mark.parametrize("form", ("u1", "S", "V"))
def test_records_keyed_by_a_byte_string(gpu, N, form):
    rng = np.random.default_rng(N * 7 + len(form))
    for n in (0, 1, 2, 3, 1_000, 100_003):
        dt = _record_dtype(N, form)
        raw = np.zeros(n * dt.itemsize, dtype=np.uint8)
        arr = raw.view(dt)
        keys = _rows(rng, n, N)
        keys[:, 0] &= 3
        keys[1::3] = keys[0::3][: keys[1::3].shape[0]]  # equal keys that must keep their input order
        b = arr.view(np.uint8).reshape(n, dt.itemsize)
        b[:, 1:1 + N] = keys
        arr["seq"] = np.arange(n, dtype=np.uint32)
        arr["tag"] = np.arange(n, dtype=np.uint64).astype(np.uint8)
        order = np.lexsort(keys.T[::-1]) if n else np.arange(0)
        exp = b[order].copy()  # whole rows from the raw bytes: indexing the structured array would drop the padding byte
        gpu.sort_host_records(arr, "k")
        assert np.array_equal(b, exp), (N, form, n)


def test_full_size_24_byte_rows(gpu):
    """10^8 rows of [u8; 24] on the device entry, checked in chunks on the host: non-decreasing rows, and the same multiset
    (order-independent row hash: sum and xor)."""
    import torch
    n, N = 100_000_000, 24
    g = torch.Generator(device="cuda")
    g.manual_seed(24)
    t = torch.randint(0, 256, (n, N), dtype=torch.uint8, device="cuda", generator=g)
    t[:, :2] = 0  # ties in the first 8 bytes, so that a refinement round runs at this size
    mult = np.array([0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9], dtype=np.uint64)

    def words(chunk):
        return chunk.view(">u8").astype(np.uint64)

    def row_hash(w):
        with np.errstate(over="ignore"):
            h = w * mult
            h = h[:, 0] + h[:, 1] + h[:, 2]
            return h ^ (h >> np.uint64(29))

    def digest(tensor, check_order):
        s, x, prev, step = np.uint64(0), np.uint64(0), None, 10_000_000
        for i in range(0, n, step):
            w = words(tensor[i:i + step].cpu().numpy())
            if check_order:
                if prev is not None:
                    w_all = np.concatenate([prev, w])
                else:
                    w_all = w
                a, b = w_all[:-1], w_all[1:]
                ok = (b[:, 0] > a[:, 0]) | ((b[:, 0] == a[:, 0]) & ((b[:, 1] > a[:, 1]) | ((b[:, 1] == a[:, 1]) & (b[:, 2] >= a[:, 2]))))
                assert ok.all(), f"rows out of order near {i}"
                prev = w[-1:]
            h = row_hash(w)
            with np.errstate(over="ignore"):
                s = s + np.sum(h, dtype=np.uint64)
            x = x ^ np.bitwise_xor.reduce(h)
        return s, x

    before = digest(t, False)
    gpu.radix_sort_unstable(t, key="bytes")
    torch.cuda.synchronize()
    after = digest(t, True)
    assert before == after
