"""Inputs shared by tests/test_gpu_segments_offsets.py and tests/test_segments_offsets_inputs.py (no tests here): the limits
pairs, and the seeded many-segment table the device plan's parity test runs on."""
import numpy as np

HEAD_GAP, TAIL_GAP = 5, 7
LIMIT_PAIRS = ((1, 0), (4, 0), (8, 0), (16, 0), (4, 4), (8, 8))     # (key bytes, value bytes)
KEY_OF_WIDTH = {1: "uint8", 2: "uint16", 4: "uint32", 8: "uint64", 16: "u128"}
MANY_SEGMENTS = 70_001
MANY_FULL_BLOCKS = 40          # segments of exactly block_max keys
MANY_MAX_KEYS = 4_000_000


def many_lengths(wave_max, block_max, seed=41):
    """70 001 lengths from {0, 1, 2, 5, wave_max, wave_max + 1, 600, block_max} plus three long ones.  The draw is weighted
    towards the short lengths so that the total stays below 4 * 10^6 keys; the lengths wave_max + 1 and 600 occur about
    1 400 times each: ties of the block class, whose order in the work list is the pair sort's stability."""
    rng = np.random.default_rng(seed)
    pool = np.array([0, 1, 2, 5, wave_max, wave_max + 1, 600], dtype=np.int64)
    lengths = rng.choice(pool, size=MANY_SEGMENTS, p=[0.25, 0.15, 0.27, 0.27, 0.02, 0.02, 0.02])
    spots = rng.choice(MANY_SEGMENTS, size=MANY_FULL_BLOCKS + 3, replace=False)
    lengths[spots[:MANY_FULL_BLOCKS]] = block_max
    lengths[spots[MANY_FULL_BLOCKS:]] = [block_max + 1, 2 * block_max + 17, block_max + 7]
    return lengths


def offsets_of(lengths):
    """(offsets, n): the borders of segments of these lengths behind a head gap, and an array length that leaves a tail gap"""
    off = HEAD_GAP + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return off, int(off[-1]) + TAIL_GAP


def class_counts(lengths, wave_max, block_max):
    """(wave, block, long) counts and the longest long segment, from the lengths alone"""
    lengths = np.asarray(lengths)
    wave = int(((lengths >= 2) & (lengths <= wave_max)).sum())
    block = int(((lengths > wave_max) & (lengths <= block_max)).sum())
    long = lengths[lengths > block_max]
    return (wave, block, len(long)), int(long.max()) if len(long) else 0
