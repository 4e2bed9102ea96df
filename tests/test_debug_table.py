"""The table of debug switches (include/itm_debug.h: itm_debug_set / itm_debug_get) and the dispatch of itm_debug_counter, host only:
the keys of the header are distinct and below ITM_DEBUG_KEY_COUNT, every key starts at its default and reads back what was stored,
numbers that are no key are refused by both calls, and the counters refuse an unknown number and a null handle."""
import ctypes as C
import os
import re
import shutil

import pytest

import itm_testlib as T
from infinitam_amd import capi

ERR_INVALID = -1
NOT_KEYS = ("ORDERED_GUARD", "KEY_COUNT")
DEFAULTS = {"EXCHANGE_CORRUPT_WORD": -1}      # every other key starts at 0
REFUSED = (0, 21, 22, 23, 32, -1)


def header_defines():
    text = open(os.path.join(T.ROOT, "include", "itm_debug.h")).read()
    return {name: int(number) for name, number in re.findall(r"^#define ITM_DEBUG_(\w+) (-?\d+)\b", text, re.M)}


@pytest.fixture(scope="module")
def keys():
    return {name: number for name, number in header_defines().items() if name not in NOT_KEYS}


@pytest.fixture(scope="module")
def fresh(tmp_path_factory):
    """A copy of the library that nothing else in this process has loaded: its switches are as the library starts."""
    import infinitam_amd
    if not os.path.exists(infinitam_amd.lib_path()):
        infinitam_amd.build()
    copy = tmp_path_factory.mktemp("debug_table") / "libitmhip_fresh.so"
    shutil.copy(infinitam_amd.lib_path(), copy)
    return capi.Backend(str(copy), "itm_")


def last_error(be):
    return (be.fn["last_error"]() or b"").decode()


def get(be, key):
    value = C.c_int(12345)
    be.check(be.fn["debug_get"](key, C.byref(value)), "debug_get")
    return value.value


def test_header_keys_are_distinct_and_below_the_count(keys):
    count = header_defines()["KEY_COUNT"]
    assert count == 32
    assert len(keys) == 28
    assert len(set(keys.values())) == len(keys), "a key number is used twice"
    assert all(0 < number < count for number in keys.values())
    assert not set(keys.values()) & set(REFUSED)
    text = open(os.path.join(T.ROOT, "include", "itm_debug.h")).read()
    order = [int(n) for name, n in re.findall(r"^#define ITM_DEBUG_(\w+) (-?\d+)\b", text, re.M) if name not in NOT_KEYS]
    assert order == sorted(order), "the keys stand in numeric order"


def test_every_key_starts_at_its_default(fresh, keys):
    for name, key in keys.items():
        assert get(fresh, key) == DEFAULTS.get(name, 0), name


def test_set_then_get_round_trips_every_key(fresh, keys):
    for name, key in keys.items():
        before = get(fresh, key)
        stored = 0 if name == "FAIL_ALLOCATION" else 7      # (a countdown of 7 would fail a later allocation of this process)
        try:
            fresh.check(fresh.fn["debug_set"](key, stored), "debug_set")
            assert get(fresh, key) == stored, name
        finally:
            fresh.check(fresh.fn["debug_set"](key, before), "debug_set")
        assert get(fresh, key) == before, name


@pytest.mark.parametrize("key", REFUSED)
def test_numbers_that_are_no_key_are_refused(fresh, key):
    assert fresh.fn["debug_set"](key, 1) == ERR_INVALID
    assert last_error(fresh) == "unknown debug key"
    fresh.fn["debug_get"](1, C.byref(C.c_int()))      # a call that succeeds in between: the next text is the next call's
    value = C.c_int(12345)
    assert fresh.fn["debug_get"](key, C.byref(value)) == ERR_INVALID
    assert last_error(fresh) == "unknown debug key"
    assert value.value == 12345


def test_unknown_counter_is_refused(fresh):
    old = C.c_uint32()
    assert fresh.fn["debug_counter"](99, None, None, C.byref(old)) == ERR_INVALID
    assert last_error(fresh) == "unknown counter"


@pytest.mark.parametrize("which", ["COUNTER_COLOUR_SEQ", "COUNTER_REN_SEQ", "COUNTER_POSE_QUALITY_SEQ", "COUNTER_ALIGN_SEQ"])
def test_null_handle_is_refused(fresh, which):
    old = C.c_uint32()
    assert fresh.fn["debug_counter"](getattr(capi, which), None, None, C.byref(old)) == ERR_INVALID
    assert last_error(fresh) == "null handle"
