"""tests/dropout_ref.py (the host restatement of csrc/mtts_common.h dropout_keep / dropout_scale) on its own:
the documented keep rate, the scale as its inverse, and the column pairing of the hash."""
from __future__ import annotations

import math

import dropout_ref as DR
import numpy as np
import pytest


@pytest.mark.parametrize("p", [0.05, 0.1, 0.19, 0.3])
def test_keep_rate_scale_and_column_pairs(p):
    rows, cols = np.arange(2048), np.arange(2048)
    seed = (987654321, 12345)
    keep = DR.keep_mask(seed, rows, cols, p)
    assert keep.dtype == np.bool_ and keep.shape == (2048, 2048)
    thresh = math.ceil(float(np.float32(p)) * 65536)
    want = (65536 - thresh) / 65536
    sd = math.sqrt(want * (1 - want) / keep.size)
    assert abs(keep.mean() - want) < 5 * sd, (keep.mean(), want)
    # the scale is the exact inverse of the keep rate (both are ratios of small integers)
    assert DR.keep_scale(p) == 65536 / (65536 - thresh)
    assert abs(DR.keep_scale(p) * want - 1.0) < 1e-15
    assert DR.keep_scale(0.0) == 1.0
    # columns 2j and 2j+1 read the low and the high half of ONE hash word: an element is kept iff its
    # 16-bit half is at least the threshold
    x = DR.keep_hash(seed, rows, cols)
    assert np.array_equal(x[:, 0::2], x[:, 1::2])
    assert np.array_equal(keep[:, 0::2], (x[:, 0::2] & np.uint32(0xFFFF)) >= thresh)
    assert np.array_equal(keep[:, 1::2], (x[:, 1::2] >> np.uint32(16)) >= thresh)
    assert not np.array_equal(keep[:, 0::2], keep[:, 1::2])


def test_keys_are_arbitrary_integers_mod_2_32():
    """Row / column keys need not be arange: any integer array, wrapped mod 2^32; the seed words are bit
    patterns (a negative int32 is its two's complement); a known value pins the arithmetic."""
    rows = np.array([0, 70000, 2 ** 32 + 5, 5, 2 ** 31 + 9])
    cols = np.array([7, 0, 129, 2 ** 32 + 7])
    a = DR.keep_mask((-5, -2 ** 31), rows, cols, 0.3)
    b = DR.keep_mask((2 ** 32 - 5, 2 ** 31), rows, cols, 0.3)
    assert np.array_equal(a, b)
    assert np.array_equal(a[2], a[3]) and np.array_equal(a[:, 0], a[:, 3])
    full = DR.keep_mask((1, 2), np.arange(70001), np.arange(130), 0.3)
    assert np.array_equal(full[np.ix_([0, 70000, 5], [7, 0, 129])], DR.keep_mask((1, 2), [0, 70000, 5], [7, 0, 129], 0.3))
    # one hand-computed word: row 1, column pair 0, seed (0, 0)
    x = (0x9E3779B1 ^ ((0x7F4A7C15 * 0x85EBCA77) % 2 ** 32)) % 2 ** 32
    x ^= x >> 16
    x = x * 0x85EBCA6B % 2 ** 32
    x ^= x >> 13
    x = x * 0xC2B2AE35 % 2 ** 32
    x ^= x >> 16
    assert int(DR.keep_hash((0, 0), [1], [0])[0, 0]) == x
