"""The inputs of tests/test_gpu_segments_offsets.py, checked where no device is needed: the seeded many-segment table holds,
for every limits pair, every class, block-class ties, empty and one-key segments, and the class counts the GPU test
asserts — computed here through rdst_segments_plan."""
import numpy as np
import pytest

from segments_offsets_inputs import (KEY_OF_WIDTH, LIMIT_PAIRS, MANY_FULL_BLOCKS, MANY_MAX_KEYS, MANY_SEGMENTS, class_counts, many_lengths,
                                     offsets_of)


@pytest.mark.parametrize("kb,vb", LIMIT_PAIRS)
def test_many_segment_table(hiplib, kb, vb):
    import rdst_amd
    key = KEY_OF_WIDTH[kb]
    wave_max, block_max = rdst_amd.segments_limits(key, vb)
    lengths = many_lengths(wave_max, block_max)
    assert len(lengths) == MANY_SEGMENTS
    off, n = offsets_of(lengths)
    assert n < MANY_MAX_KEYS and n < 2**31                      # int32 offsets can hold it
    assert (lengths == 0).sum() > 1000 and (lengths == 1).sum() > 1000
    for value in (2, 5, wave_max, wave_max + 1, 600, block_max, block_max + 1, block_max + 7, 2 * block_max + 17):
        assert (lengths == value).any(), value
    items, counts, tmp_elems = rdst_amd.segments_plan(off, n, key, vb)
    expect, longest = class_counts(lengths, wave_max, block_max)
    assert counts == expect and tmp_elems == longest == 2 * block_max + 17
    assert min(counts) > 0 and counts[2] == 3                   # every class
    assert (lengths == block_max).sum() == MANY_FULL_BLOCKS
    # the pair sort of the plan takes several tiles per pass (the largest pair tile is 8 448 pairs)
    assert MANY_SEGMENTS > 8 * 8448
    # block-class ties: neighbours in the work list with one length, which must stand in segment order
    block = items[counts[0]:counts[0] + counts[1]]
    ties = sum(1 for a, b in zip(block, block[1:]) if a[1] == b[1])
    assert ties >= 100
    assert all(a[2] < b[2] for a, b in zip(block, block[1:]) if a[1] == b[1])
    assert [it[1] for it in block] == sorted((it[1] for it in block), reverse=True)
    # the wave and the long class stand in segment order
    for part in (items[:counts[0]], items[counts[0] + counts[1]:]):
        assert all(a[2] < b[2] for a, b in zip(part, part[1:]))
    assert len({it[1] for it in block}) >= 3                    # wave_max + 1, 600 (one of them twice for no width) and block_max
