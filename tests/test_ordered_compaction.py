"""The ordered compaction (csrc/ordered_device.h, launch_ordered_compaction) in isolation, through itm_debug_ordered_compact: the
list is np.flatnonzero(flags)[:cap], the counts are np.count_nonzero(flags) and its minimum with cap -- for byte flags (the hash
callers: visible list, FindVisibleBlocks, the mesher's slot list; multiples of 8) and int32 flags (the pixel callers; any number).
The hook uploads the caller's ids array, guard words included, as the device list before the launch and downloads all of it after,
so the sentinel assertions below see device memory: every word the launch did not list must still hold the sentinel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 2048
SENTINEL = -7
GUARD = 8                  # ITM_DEBUG_ORDERED_GUARD (include/itm_debug.h)
DTYPES = [np.uint8, np.int32]


def compact(hip, flags, cap=None):
    """ids (cap + GUARD long, pre-filled with SENTINEL; the device list's contents before and after) and [raw total, total after the cap]"""
    flags = np.ascontiguousarray(flags)
    cap = flags.size if cap is None else cap
    ids = np.full(cap + GUARD, SENTINEL, np.int32)
    counts = np.full(2, SENTINEL, np.int32)
    hip.check(hip.fn["debug_ordered_compact"](flags.ctypes.data, flags.itemsize, flags.size, cap, ids.ctypes.data, counts.ctypes.data, None),
              "debug_ordered_compact")
    return ids, counts


def check(hip, flags, cap=None):
    ids, counts = compact(hip, flags, cap)
    cap = flags.size if cap is None else cap
    total = int(np.count_nonzero(flags))
    listed = min(total, cap)
    assert counts.tolist() == [total, listed]
    assert np.array_equal(ids[:listed], np.flatnonzero(flags)[:cap])
    assert np.all(ids[listed:] == SENTINEL)            # the launch wrote nothing at or beyond the end of the list, nor past cap


def random_flags(dtype, n, density, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(n) < density).astype(dtype)


@pytest.mark.parametrize("dtype,n", [(d, n) for d in DTYPES for n in (8, 2040, 2048, 2056)] + [(np.int32, n) for n in (1, 2047, 2049)])
def test_sizes_around_one_chunk(hip, dtype, n):
    check(hip, random_flags(dtype, n, 0.5, n))
    check(hip, np.ones(n, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_flag_leaves_the_list_untouched(hip, dtype):
    check(hip, np.zeros(5 * CHUNK, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_flag_set_with_values_other_than_one(hip, dtype):
    values = [0x80, 3, 255] if dtype is np.uint8 else [0x80, 3, 255, -1, 1 << 20, -(1 << 31)]
    check(hip, np.resize(np.array(values, dtype), 3 * CHUNK + 8))


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_chunks_between_flagged_ones(hip, dtype):
    """chunks 1, 2 and 3 leave early; chunk 4's base is chunk 0's count"""
    flags = np.zeros(5 * CHUNK, dtype)
    flags[:CHUNK] = random_flags(dtype, CHUNK, 0.3, 1)
    flags[4 * CHUNK:] = random_flags(dtype, CHUNK, 0.3, 2)
    check(hip, flags)


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_chunks_than_lanes(hip, dtype):
    """301 chunks: the base loop strides; flags only in the first and last element of chunks 0, 255, 256, 257 and the last (short) one"""
    n = 300 * CHUNK + 8
    flags = np.zeros(n, dtype)
    for c in (0, 255, 256, 257):
        flags[c * CHUNK] = flags[c * CHUNK + CHUNK - 1] = 1
    flags[300 * CHUNK] = flags[n - 1] = 1
    check(hip, flags)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("density", [0.01, 0.5])
def test_random_flags(hip, dtype, density):
    check(hip, random_flags(dtype, 5 * CHUNK, density, 11))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cap", ["total - 1", 1, 0])
def test_list_shorter_than_the_flags(hip, dtype, cap):
    """the raw total is unchanged, the capped total equals cap, nothing is written at or beyond cap"""
    flags = random_flags(dtype, 5 * CHUNK, 0.5, 11)
    total = int(np.count_nonzero(flags))
    cap = total - 1 if cap == "total - 1" else cap
    assert cap < total
    check(hip, flags, cap)
