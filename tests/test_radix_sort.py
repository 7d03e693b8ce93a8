"""The detection's own radix sort (dem-engine_amd/csrc/deme_sort.h), alone, through deme_sort_pairs_u32 / deme_sort_keys_u64.

The reference is numpy's stable argsort of the key's bits [beginBit, endBit): a stable sort has one answer, so the comparison
is equality.  The values are 0 .. n-1, so they show the order equal digits came out in; the keys carry random bits outside the
sorted range, which must neither move an entry nor change on the way."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ["random", "equal", "sorted", "reversed", "three"]
# [0, 1); a last digit narrower than the others (21 = 8 + 8 + 5, 22 = 8 + 8 + 6); exactly one digit, at bit 0 and above it; and
# the contact keys' range, which only 64-bit keys have
RANGES_U32 = [(0, 1), (0, 21), (0, 22), (0, 8), (13, 21)]
RANGES_U64 = RANGES_U32 + [(31, 55)]


def _sizes(pkg):
    t = pkg.abi.sort_tile_keys()
    return [0, 1, 2, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 3 * t + 1, 65537, 300001]


def _field(kind, n, width, rng):
    """n values of `width` bits: the part of the keys the sort looks at"""
    top = 1 << width
    if kind == "random":
        return rng.integers(0, top, n, dtype=np.uint64)
    if kind == "equal":
        return np.full(n, rng.integers(0, top), np.uint64)
    if kind == "sorted":
        return np.sort(rng.integers(0, top, n, dtype=np.uint64))
    if kind == "reversed":
        return np.sort(rng.integers(0, top, n, dtype=np.uint64))[::-1].copy()
    if kind == "three":
        some = rng.choice(top, size=min(3, top), replace=False).astype(np.uint64)
        return some[rng.integers(0, len(some), n)]
    raise ValueError(kind)


def _keys(kind, n, b0, b1, dtype, rng):
    """the field at [b0, b1), random bits everywhere else"""
    bits = np.dtype(dtype).itemsize * 8
    inside = ((1 << (b1 - b0)) - 1) << b0
    junk = rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
    k = (junk & np.uint64(~inside & ((1 << bits) - 1))) | (_field(kind, n, b1 - b0, rng) << np.uint64(b0))
    return k.astype(dtype)


def _order(keys, b0, b1):
    return np.argsort((keys.astype(np.uint64) >> np.uint64(b0)) & np.uint64((1 << (b1 - b0)) - 1), kind="stable")


def _check_pairs(pkg, keys, b0, b1, force_own, what):
    vals = np.arange(keys.size, dtype=np.uint32)
    ko, vo = pkg.abi.sort_pairs_u32(keys, vals, b0, b1, force_own=force_own)
    order = _order(keys, b0, b1)
    assert np.array_equal(vo, vals[order]), f"{what}: values (the order of the entries)"
    assert np.array_equal(ko, keys[order]), f"{what}: keys"


def _check_keys(pkg, keys, b0, b1, force_own, what):
    ko = pkg.abi.sort_keys_u64(keys, b0, b1, force_own=force_own)
    assert np.array_equal(ko, keys[_order(keys, b0, b1)]), f"{what}: keys"


def test_sort_entry_points_are_exported_and_bound(pkg):
    names = pkg.abi.exported_symbols()
    lib = pkg.abi.load_library()
    for n in ("deme_sort_pairs_u32", "deme_sort_keys_u64", "deme_sort_tile_keys"):
        assert n in names and hasattr(lib, n), n
    t = pkg.abi.sort_tile_keys()
    assert t >= 256 and t % 64 == 0


@pytest.mark.parametrize("kind", KINDS)
def test_own_sort_pairs_u32(pkg, kind):
    rng = np.random.default_rng(KINDS.index(kind))
    for n in _sizes(pkg):
        for b0, b1 in RANGES_U32:
            _check_pairs(pkg, _keys(kind, n, b0, b1, np.uint32, rng), b0, b1, True, f"{kind} keys, n {n}, bits [{b0}, {b1})")


@pytest.mark.parametrize("kind", KINDS)
def test_own_sort_keys_u64(pkg, kind):
    rng = np.random.default_rng(100 + KINDS.index(kind))
    for n in _sizes(pkg):
        for b0, b1 in RANGES_U64:
            _check_keys(pkg, _keys(kind, n, b0, b1, np.uint64, rng), b0, b1, True, f"{kind} keys, n {n}, bits [{b0}, {b1})")


def test_u64_values_identify_entries_with_equal_fields(pkg):
    """Keys alone cannot show a lost order -- unless the bits outside the range differ, which they do: with a constant field
    the output must be the input, entry by entry."""
    rng = np.random.default_rng(7)
    keys = _keys("equal", 3 * pkg.abi.sort_tile_keys() + 1, 31, 55, np.uint64, rng)
    assert len(np.unique(keys)) > keys.size // 2
    assert np.array_equal(pkg.abi.sort_keys_u64(keys, 31, 55, force_own=True), keys)


# what the detection's call sites take: rocprim for a small list, the own sort for a large one
@pytest.mark.parametrize("n", [1000, 1000003])
def test_call_site_choice_on_both_sides_of_the_threshold(pkg, n):
    rng = np.random.default_rng(n)
    _check_pairs(pkg, _keys("random", n, 0, 22, np.uint32, rng), 0, 22, False, f"incidence pairs, n {n}")
    _check_pairs(pkg, _keys("random", n, 0, 20, np.uint32, rng), 0, 20, False, f"crossing-record pairs, n {n}")
    _check_keys(pkg, _keys("random", n, 31, 55, np.uint64, rng), 31, 55, False, f"contact keys, n {n}")
