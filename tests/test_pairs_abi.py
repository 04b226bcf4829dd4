"""CPU-side checks of the key-value entry point (rdst_hip_sort_pairs_device): every argument error returns before any device
work, with the status the header names.  Where two rules collide the header leaves the order open; the order asserted here is
the one the code applies."""
import ctypes

OK, ERR_ARG, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3


def _pointers():
    """four made-up 'device' pointers, 16-byte aligned (host memory: no call below gets as far as a device)"""
    bufs = [(ctypes.c_uint8 * 4096)() for _ in range(4)]
    ptrs = [(ctypes.cast(b, ctypes.c_void_p).value + 15) // 16 * 16 for b in bufs]
    return bufs, ptrs


def _call(lib, k, v, tk, tv, n, kb, kind, levels, vb):
    vp = ctypes.c_void_p
    return lib.rdst_hip_sort_pairs_device(vp(k), vp(v), vp(tk), vp(tv), n, kb, kind, levels, vb, None)


def test_key_and_value_widths(hiplib):
    _keep, (k, v, tk, tv) = _pointers()
    for kb in (1, 2, 16):                                    # widths the key-only sorts take, the key-value sort does not
        assert _call(hiplib, k, v, tk, tv, 8, kb, UNSIGNED, kb, 4) == ERR_UNSUPPORTED, kb
        assert b"4- or 8-byte keys" in hiplib.rdst_hip_last_error()
    for kb in (0, 3, 5, 12, 32):                             # widths nothing is built for
        assert _call(hiplib, k, v, tk, tv, 8, kb, UNSIGNED, kb, 4) == ERR_UNSUPPORTED, kb
    for kb in (4, 8):
        for vb in (0, 1, 2, 3, 5, 12, 16):
            assert _call(hiplib, k, v, tk, tv, 8, kb, UNSIGNED, kb, vb) == ERR_UNSUPPORTED, (kb, vb)
            assert b"values" in hiplib.rdst_hip_last_error()
    assert _call(hiplib, k, v, tk, tv, 8, 2, FLOAT, 2, 4) == ERR_UNSUPPORTED      # no 2-byte float key either


def test_levels_and_kinds(hiplib):
    _keep, (k, v, tk, tv) = _pointers()
    for kb in (4, 8):
        assert _call(hiplib, k, v, tk, tv, 8, kb, UNSIGNED, 0, 4) == ERR_ARG      # LEVELS == 0 (src/radix_sort_builder.rs:22)
        assert b"level" in hiplib.rdst_hip_last_error()
        for levels in (1, kb - 1, kb + 1, 16):
            assert _call(hiplib, k, v, tk, tv, 8, kb, SIGNED, levels, 8) == ERR_ARG, (kb, levels)
        assert _call(hiplib, k, v, tk, tv, 8, kb, BYTES_BE, kb, 4) == ERR_UNSUPPORTED
        for kind in (4, 7, -1):
            assert _call(hiplib, k, v, tk, tv, 8, kb, kind, kb, 4) == ERR_ARG, kind
            assert b"kind" in hiplib.rdst_hip_last_error()


def test_key_pointer(hiplib):
    _keep, (k, v, tk, tv) = _pointers()
    assert _call(hiplib, None, v, tk, tv, 8, 4, UNSIGNED, 4, 4) == ERR_ARG
    assert b"null key" in hiplib.rdst_hip_last_error()
    assert _call(hiplib, k + 2, v, tk, tv, 8, 4, UNSIGNED, 4, 4) == ERR_ALIGN
    assert _call(hiplib, k + 4, v, tk, tv, 8, 8, UNSIGNED, 8, 4) == ERR_ALIGN
    assert _call(hiplib, k, v, tk, tv, 1 << 36, 4, UNSIGNED, 4, 4) == ERR_ARG     # len too large


def test_short_slices_need_no_values_and_no_tmps(hiplib):
    _keep, (k, v, tk, tv) = _pointers()
    for n in (0, 1):
        for kb in (4, 8):
            for vb in (4, 8):
                assert _call(hiplib, k, None, None, None, n, kb, FLOAT, kb, vb) == OK, (n, kb, vb)
    assert _call(hiplib, None, None, None, None, 0, 4, UNSIGNED, 4, 4) == OK       # an empty slice may be a null pointer
    assert _call(hiplib, k, v + 1, tk + 1, tv + 1, 1, 8, UNSIGNED, 8, 8) == OK     # nor are the other pointers looked at


def test_value_and_tmp_pointers(hiplib):
    _keep, (k, v, tk, tv) = _pointers()
    for n in (2, 1000):
        assert _call(hiplib, k, None, tk, tv, n, 4, UNSIGNED, 4, 4) == ERR_ARG
        assert _call(hiplib, k, v, None, tv, n, 4, UNSIGNED, 4, 4) == ERR_ARG
        assert _call(hiplib, k, v, tk, None, n, 4, UNSIGNED, 4, 4) == ERR_ARG
        assert b"null value / tmp" in hiplib.rdst_hip_last_error()
        for kb, vb in ((4, 4), (4, 8), (8, 4), (8, 8)):
            assert _call(hiplib, k, v, tk + kb // 2, tv, n, kb, SIGNED, kb, vb) == ERR_ALIGN, (kb, vb)
            assert b"tmp key" in hiplib.rdst_hip_last_error()
            assert _call(hiplib, k, v + vb // 2, tk, tv, n, kb, SIGNED, kb, vb) == ERR_ALIGN, (kb, vb)
            assert _call(hiplib, k, v, tk, tv + vb // 2, n, kb, SIGNED, kb, vb) == ERR_ALIGN, (kb, vb)
            assert b"value pointer" in hiplib.rdst_hip_last_error()
        # element alignment is all that is asked: 4 bytes past a 16-byte boundary is fine for 4-byte elements only
        assert _call(hiplib, k, v + 4, tk, tv, n, 4, UNSIGNED, 4, 8) == ERR_ALIGN
        assert _call(hiplib, k, v, tk + 4, tv, n, 8, UNSIGNED, 8, 4) == ERR_ALIGN


def test_order_of_colliding_rules(hiplib):
    """the order the code applies today (the header leaves it open): the checks shared with the key-only entry first — width,
    levels, kind, key pointer — then the pair widths, the short-slice return, null pointers, alignment"""
    _keep, (k, v, tk, tv) = _pointers()
    assert _call(hiplib, k, v, tk, tv, 8, 3, UNSIGNED, 0, 4) == ERR_UNSUPPORTED    # width before levels
    assert _call(hiplib, k, v, tk, tv, 8, 2, UNSIGNED, 0, 4) == ERR_ARG            # levels before the pair key widths
    assert _call(hiplib, k, v, tk, tv, 8, 4, BYTES_BE, 3, 4) == ERR_ARG            # levels before the kind
    assert _call(hiplib, None, v, tk, tv, 8, 4, 9, 4, 4) == ERR_ARG                # (kind and null keys: both ERR_ARG)
    assert b"kind" in hiplib.rdst_hip_last_error()
    assert _call(hiplib, k + 8, v, tk, tv, 8, 16, UNSIGNED, 16, 4) == ERR_ALIGN    # key alignment before the pair key widths
    assert _call(hiplib, k + 2, v, tk, tv, 8, 4, UNSIGNED, 4, 3) == ERR_ALIGN      # ... and before the value width
    assert _call(hiplib, k, v, tk, tv, 1, 2, UNSIGNED, 2, 4) == ERR_UNSUPPORTED    # widths before the short-slice return
    assert _call(hiplib, k, None, None, None, 0, 4, UNSIGNED, 4, 16) == ERR_UNSUPPORTED
    assert _call(hiplib, None, None, None, None, 1, 4, UNSIGNED, 4, 4) == ERR_ARG  # null keys with len 1: before that return
    assert _call(hiplib, k, None, tk + 2, tv, 8, 4, UNSIGNED, 4, 4) == ERR_ARG     # null pointers before alignment
    assert _call(hiplib, k, v + 2, tk + 2, tv, 8, 4, UNSIGNED, 4, 4) == ERR_ALIGN
    assert b"tmp key" in hiplib.rdst_hip_last_error()                              # tmp keys before the value pointers
