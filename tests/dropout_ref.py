"""Host restatement of the counter-based dropout mask (csrc/mtts_common.h: dropout_keep / dropout_scale)
in numpy uint32 / float32 -- test infrastructure only.  The mask is a pure function of the two seed words,
the (row, column) key and p, so every kernel that drops can be checked element by element."""
from __future__ import annotations

import math

import numpy as np

_U = np.uint32


def _words(seed_words):
    """The two 32-bit seed words as the kernels read them: a torch int32 tensor (device or host), a numpy
    array or a pair of Python ints; negative int32 values are their two's-complement bit patterns."""
    if hasattr(seed_words, "detach"):
        seed_words = seed_words.detach().cpu().numpy()
    lo, hi = (int(v) & 0xFFFFFFFF for v in np.asarray(seed_words).reshape(-1)[:2].tolist())
    return _U(lo), _U(hi)


def keep_hash(seed_words, rows, cols) -> np.ndarray:
    """The hash word of each (row, column pair): uint32 [len(rows), len(cols)]."""
    lo, hi = _words(seed_words)
    r = (np.asarray(rows).astype(np.int64) & 0xFFFFFFFF).astype(_U).reshape(-1, 1)
    c = (np.asarray(cols).astype(np.int64) & 0xFFFFFFFF).astype(_U).reshape(1, -1)
    with np.errstate(over="ignore"):
        x = ((r * _U(0x9E3779B1)) ^ (((c >> _U(1)) + _U(0x7F4A7C15)) * _U(0x85EBCA77)) ^ lo) + hi
        x = x ^ (x >> _U(16))
        x = x * _U(0x85EBCA6B)
        x = x ^ (x >> _U(13))
        x = x * _U(0xC2B2AE35)
        x = x ^ (x >> _U(16))
    return x


def keep_mask(seed_words, rows, cols, p) -> np.ndarray:
    """bool [len(rows), len(cols)]: element (rows[i], cols[j]) survives dropout(p).  rows / cols are the
    integer keys the kernel hashes (any integer arrays, taken mod 2^32)."""
    x = keep_hash(seed_words, rows, cols)
    odd = (np.asarray(cols).astype(np.int64).reshape(1, -1) & 1).astype(bool)
    u = np.where(odd, x >> _U(16), x & _U(0xFFFF))
    return u.astype(np.float32) * np.float32(2.0 ** -16) >= np.float32(p)


def keep_scale(p) -> float:
    """1 / P(keep): 65536 / (65536 - ceil(float32(p) * 65536)); 1 at p <= 0.  (Exact in float32 up to the
    final division, which the caller rounds: np.float32(keep_scale(p)) is the kernels' factor.)"""
    p32 = np.float32(p)
    if not p32 > 0:
        return 1.0
    return 65536.0 / (65536.0 - math.ceil(float(p32) * 65536.0))
