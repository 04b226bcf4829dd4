"""Inputs of the nowait [u8; N] and described-key tests (rdst_hip_sort_bytes_device_nowait,
rdst_hip_sort_records_by_fields_device_nowait): the round loop of bytes_order_nowait restated in numpy, the
row families that leave its tie flag down or raise it, and the field tables of the records cases.  Shared by the CPU test
of the inputs (tests/test_bytes_nowait_inputs.py) and the GPU tests, so that both see the same rows."""
import functools

import numpy as np

UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
NOWAIT_MAX_N = 128
GRID_ROWS = 256 * 16 * 256       # rows one trip of tie_flag_kernel covers: GRID_CAP workgroups of 256 items

WIDE_WIDTHS = (17, 24, 25, 32, 64, 128)      # 17: a one-byte last chunk; 24, 32, 64, 128: whole chunks; 25: one byte past
FORWARDED_WIDTHS = (3, 16)
CPU_WIDTHS = (9, 16, 17, 24, 25, 32, 128)
CPU_LENGTHS = (2, 3, 300, 5_377)
FLAG_UP_FAMILIES = ("last byte", "middle chunk", "all equal", "three rows")


def lengths(pair_tile):
    """the row counts of the GPU tests, around the pair sort's tile (helpers.pair_tile(8, 4))"""
    return 2, 3, 300, pair_tile - 1, pair_tile, pair_tile + 1, 70_001


def chunk_keys(rows, c):
    """big-endian u64 of bytes [8c, min(8c + 8, N)) of every row, left-justified, zero-filled"""
    n, N = rows.shape
    part = rows[:, 8 * c:min(8 * c + 8, N)]
    buf = np.zeros((n, 8), dtype=np.uint8)
    buf[:, :part.shape[1]] = part
    return buf.view(">u8").ravel().astype(np.uint64)


def nowait_order(rows):
    """bytes_order_nowait in numpy: (row indices in output order, tie flag).  The prefix pair sort, the flag, then
    ceil(N / 8) rounds, last chunk first, each a stable sort of (chunk key or 0, row)."""
    n, N = rows.shape
    prefix = chunk_keys(rows, 0)
    idx = np.argsort(prefix, kind="stable")
    keys = prefix[idx]
    flag = bool((keys[1:] == keys[:-1]).any())
    for c in reversed(range(-(-N // 8))):
        key = chunk_keys(rows, c)[idx] if flag else np.zeros(n, dtype=np.uint64)
        idx = idx[np.argsort(key, kind="stable")]
    return idx, flag


def stable_order(keys):
    """the stable lexicographic order of the rows of an (n, L) uint8 matrix"""
    return np.lexsort(keys.T[::-1])


def family(name, n, N, seed=0):
    """(n, N) uint8 rows.  "random": flag down (no two 8-byte prefixes collide at these n); the others raise it:
    "last byte" rows share bytes [0, N - 1); "middle chunk" rows differ only inside one chunk, which for N > 16 is neither
    the prefix nor the last; "all equal"; "three rows": three distinct rows with one prefix, repeated."""
    rng = np.random.default_rng([seed, n, N, sorted(FLAG_UP_FAMILIES + ("random",)).index(name)])
    if name == "random":
        return rng.integers(0, 256, size=(n, N), dtype=np.uint8)
    base = rng.integers(0, 256, size=N, dtype=np.uint8)
    rows = np.tile(base, (n, 1))
    if name == "last byte":
        rows[:, N - 1] = rng.integers(0, 256, size=n, dtype=np.uint8)
    elif name == "middle chunk":
        c = max(1, (-(-N // 8) - 1) // 2)
        lo, hi = 8 * c, min(8 * c + 8, N)
        rows[:, lo:hi] = rng.integers(0, 4, size=(n, hi - lo), dtype=np.uint8) * 85     # few values: equal rows occur as well
    elif name == "three rows":
        three = rng.integers(0, 256, size=(3, N), dtype=np.uint8)
        three[:, :8] = base[:8]                         # the same prefix: the later chunks decide
        three[:, N - 1] = (7, 5, 6)                     # distinct whatever the random bytes are
        rows = three[rng.integers(0, 3, size=n)]
    else:
        assert name == "all equal", name
    return rows


def one_pair(n, N, pos, seed=0):
    """Rows whose 8-byte prefixes are distinct but for one pair: the row of rank r has the prefix (r + 1) * K, big-endian,
    except rank pos + 1, which shares that of rank pos; the bytes behind are random, and byte 8 puts rank pos before rank
    pos + 1.  In the input the row of rank pos + 1 comes BEFORE the row of rank pos, so the prefix sort alone leaves the pair
    the wrong way round.  Returns (input rows, sorted rows)."""
    assert N > 8 and 0 <= pos < n - 1
    rng = np.random.default_rng([seed, n, N, pos])
    rank = np.arange(n, dtype=np.uint64)
    rank[pos + 1] = pos
    prefix = ((rank + np.uint64(1)) * np.uint64((1 << 63) // n)).astype(">u8").view(np.uint8).reshape(n, 8)
    srt = np.concatenate([prefix, rng.integers(0, 256, size=(n, N - 8), dtype=np.uint8)], axis=1)
    srt[pos, 8], srt[pos + 1, 8] = 0x10, 0x20
    perm = rng.permutation(n)
    at = np.empty(n, dtype=np.int64)
    at[perm] = np.arange(n)                             # at[r]: where rank r stands in the input
    if at[pos] < at[pos + 1]:
        perm[[at[pos], at[pos + 1]]] = perm[[at[pos + 1], at[pos]]]
    return srt[perm], srt


# ---- records -------------------------------------------------------------------------------------------------------------
RECORD_SIZES = (24, 130)         # 256 records x 24 bytes fit the pack kernel's LDS tile (staged), x 130 bytes do not (direct)
KEY_SPAN = 20                    # every field lies inside these bytes; the last four bytes of a record are its payload
# L -> fields (offset inside the key span, bytes, kind, descending); fields overlap where L exceeds the span
FIELD_TABLES = {
    8: [(10, 4, FLOAT, 0), (0, 2, UNSIGNED, 0), (3, 2, BYTES_BE, 1)],
    9: [(0, 1, UNSIGNED, 0), (2, 8, SIGNED, 1)],
    12: [(10, 4, FLOAT, 0), (2, 8, SIGNED, 0)],
    16: [(12, 8, FLOAT, 1), (0, 2, UNSIGNED, 0), (3, 6, BYTES_BE, 0)],
    17: [(19, 1, UNSIGNED, 1), (1, 16, BYTES_BE, 0)],
    40: [(10, 4, FLOAT, 0), (0, 20, BYTES_BE, 0), (2, 8, SIGNED, 1), (12, 8, FLOAT, 0)],
    128: [(0, 20, BYTES_BE, 0)] * 4 + [(12, 8, FLOAT, 0), (2, 8, SIGNED, 1), (4, 16, BYTES_BE, 1), (0, 16, UNSIGNED, 0)],
}


def field_table(L, record_bytes):
    """FIELD_TABLES[L] placed in a record: at the record's start (24 bytes) or 101 bytes in (130 bytes: odd offsets)"""
    shift = 0 if record_bytes == 24 else 101
    assert shift + KEY_SPAN <= record_bytes - 4
    fields = [(o + shift, b, k, d) for o, b, k, d in FIELD_TABLES[L]]
    assert sum(f[1] for f in fields) == L
    return fields


def kmatrix(raw, fields):
    """K of every record (include/rdst_hip.h), (n, L) uint8: the fields' mapped values, big-endian, in field order"""
    cols = []
    for offset, nbytes, kind, desc in fields:
        b = raw[:, offset:offset + nbytes].copy()
        if kind != BYTES_BE:
            b = b[:, ::-1].copy()                       # stored little-endian
            if kind == SIGNED:
                b[:, 0] ^= 0x80
            elif kind == FLOAT:
                neg = (b[:, 0] & 0x80) != 0
                b[neg] = ~b[neg]
                b[~neg, 0] ^= 0x80
        cols.append(~b if desc else b)
    return np.concatenate(cols, axis=1)


def records(n, record_bytes, seed=0, pool=37, equal_keys=False):
    """(n, record_bytes) uint8: half of the records take their bytes from a pool of `pool` records (equal keys, tied
    prefixes), half are random; `equal_keys`: all from one.  The last four bytes hold the record's input position."""
    rng = np.random.default_rng([seed, n, record_bytes])
    raw = rng.integers(0, 256, size=(n, record_bytes), dtype=np.uint8)
    base = rng.integers(0, 256, size=(pool, record_bytes), dtype=np.uint8)
    pick = np.ones(n, dtype=bool) if equal_keys else rng.random(n) < 0.5
    raw[pick] = base[0] if equal_keys else base[rng.integers(0, pool, size=int(pick.sum()))]
    raw[:, record_bytes - 4:] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)
    return raw


@functools.lru_cache(maxsize=None)
def record_case(n, record_bytes, L, equal_keys=False):
    """(raw, fields, expected) of one records case, built once (never modified)"""
    fields = field_table(L, record_bytes)
    raw = records(n, record_bytes, seed=L, equal_keys=equal_keys)
    exp = raw[stable_order(kmatrix(raw, fields))]
    for a in (raw, exp):
        a.setflags(write=False)
    return raw, fields, exp
