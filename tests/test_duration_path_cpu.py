"""Precomputed durations as a run-length alignment: the rule (monotonic_align.duration_runs_host, the Python twin
of csrc/mas.hip duration_path_kernel) against the reference's own builder -- recorded in
tests/golden/duration_path_golden.npz by tests/golden/_duration_golden.py -- and against this package's
generate_path, bit for bit.  No GPU.

The case list (``cases()``) is shared with tests/test_duration_path_gpu.py and with the fixture's generator."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "duration_path_golden.npz"
SHAPES = [(1, 1), (5, 17), (12, 40), (257, 300)]  # 257 rows: past one row per thread of the 256-thread block
B = 3
GARBAGE = [37.0, -4.0, float("nan"), 1e9]  # what may stand past t_x: it must count for nothing


def _compose(rng, n, total):
    """n non-negative integers that add up to ``total`` (zeros allowed)."""
    cuts = np.sort(rng.randint(0, total + 1, size=n - 1))
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(np.float32)


def cases():
    """[(name, durations float32 [B,Tx], x_lengths [B], y_lengths [B], Ty)].  Per shape:
    cover   utterance 0 covers t_y exactly, 1 stops 3 frames short, 2 runs 7 frames over
    zeros   0: leading, middle and trailing rows of length 0; 1: every duration 0 (t_cov = 0); 2: exact cover;
            GARBAGE past t_x in all three (t_x < Tx in 1 and 2)
    half, x125   ``cover`` scaled by 0.5 (fractional boundaries, under-covered) and 1.25 (over-covered)
    int64, b1t   ``cover`` given as int64, ``zeros`` given as [B,1,Tx] (the values stored here stay float32)"""
    out = []
    for Tx, Ty in SHAPES:
        rng = np.random.RandomState(1000 * Tx + Ty)
        xl = np.array([Tx, max(1, Tx * 2 // 3), max(1, Tx - 1)], dtype=np.int64)
        yl = np.array([Ty, max(1, Ty * 3 // 4), max(1, Ty - 1)], dtype=np.int64)
        cover = np.zeros((B, Tx), dtype=np.float32)
        for b, total in enumerate((yl[0], max(yl[1] - 3, 0), yl[2] + 7)):
            cover[b, :xl[b]] = _compose(rng, xl[b], total)
        zeros = np.zeros((B, Tx), dtype=np.float32)
        zeros[0, :xl[0]] = _compose(rng, xl[0], yl[0])
        zeros[0, [0, xl[0] // 2, xl[0] - 1]] = 0.0
        zeros[2, :xl[2]] = _compose(rng, xl[2], yl[2])
        for b in range(B):
            n = Tx - xl[b]
            zeros[b, xl[b]:] = (GARBAGE * (n // len(GARBAGE) + 1))[:n]
        tag = f"{Tx}x{Ty}"
        out += [(f"cover_{tag}", cover, xl, yl, Ty), (f"zeros_{tag}", zeros, xl, yl, Ty),
                (f"half_{tag}", cover * np.float32(0.5), xl, yl, Ty),
                (f"x125_{tag}", cover * np.float32(1.25), xl, yl, Ty),
                (f"int64_{tag}", cover.copy(), xl, yl, Ty), (f"b1t_{tag}", zeros.copy(), xl, yl, Ty)]
    return out


CASES = cases()
_GOLD = {}


def golden():
    if not _GOLD:
        _GOLD.update(np.load(GOLDEN))
    return _GOLD


def host_rule(d, xl, yl, Ty):
    """duration_runs_host on a batch -> (path int8 [B,Tx,Ty], dur [B,Tx], col_row [B,Ty], row_start [B,Tx],
    lengths [B,2], run_lengths [B,2]) as the device op returns them."""
    from matcha.utils.monotonic_align import duration_runs_host

    nb, Tx = d.shape
    path = np.zeros((nb, Tx, Ty), dtype=np.int8)
    dur = np.zeros((nb, Tx), dtype=np.float32)
    col_row = np.full((nb, Ty), -1, dtype=np.int32)
    row_start = np.zeros((nb, Tx), dtype=np.int32)
    lengths = np.zeros((nb, 2), dtype=np.int32)
    run_lengths = np.zeros((nb, 2), dtype=np.int32)
    for b in range(nb):
        t_x, t_y = min(int(xl[b]), Tx), min(int(yl[b]), Ty)
        rs, du, cr, t_cov = duration_runs_host(d[b].tolist(), t_x, t_y)
        row_start[b], dur[b] = rs, du
        col_row[b, :t_y] = cr
        lengths[b], run_lengths[b] = (t_x, t_y), (t_x, t_cov)
        for y, x in enumerate(cr):
            if x >= 0:
                path[b, x, y] = 1
    return path, dur, col_row, row_start, lengths, run_lengths


def attn_mask(xl, yl, Tx, Ty):
    xm = (torch.arange(Tx)[None] < torch.as_tensor(xl)[:, None]).float()
    ym = (torch.arange(Ty)[None] < torch.as_tensor(yl)[:, None]).float()
    return xm[:, :, None] * ym[:, None, :]


def test_fixture_holds_every_case():
    g = golden()
    for name, d, xl, yl, Ty in CASES:
        np.testing.assert_array_equal(g[name + "_d"], d, err_msg=name)  # NaN == NaN here
        np.testing.assert_array_equal(g[name + "_xl"], xl)
        np.testing.assert_array_equal(g[name + "_yl"], yl)
        assert g[name + "_path"].shape == (B, d.shape[1], Ty) and g[name + "_path"].dtype == np.int8


@pytest.mark.parametrize("name,d,xl,yl,Ty", CASES, ids=[c[0] for c in CASES])
def test_host_rule_vs_reference_fixture_and_generate_path(name, d, xl, yl, Ty):
    from matcha.utils.model import generate_path

    path, dur, col_row, row_start, lengths, run_lengths = host_rule(d, xl, yl, Ty)
    np.testing.assert_array_equal(path, golden()[name + "_path"])
    own = generate_path(torch.from_numpy(d), attn_mask(xl, yl, d.shape[1], Ty)).numpy()
    np.testing.assert_array_equal(path, own.astype(np.int8))
    np.testing.assert_array_equal(dur, own.sum(-1))  # the duration target, attn.sum(-1)
    # the runs say the same as the dense path
    for b in range(B):
        t_x, t_cov = run_lengths[b]
        assert (row_start[b, t_x:] == -1).all() and (dur[b, t_x:] == 0).all()
        assert t_cov == int(dur[b].sum()) <= lengths[b, 1]
        np.testing.assert_array_equal(row_start[b, :t_x], np.concatenate([[0], np.cumsum(dur[b, :t_x])[:-1]]))
        assert (col_row[b, t_cov:] == -1).all()
        np.testing.assert_array_equal(col_row[b, :t_cov], path[b].argmax(0)[:t_cov])


def test_host_rule_edges():
    from matcha.utils.monotonic_align import duration_runs_host

    # NaN and negatives count as 0, +inf fills the rest, nothing reaches past t_y
    rs, du, cr, t_cov = duration_runs_host([2.0, float("nan"), -3.0, 0.5, float("inf"), 4.0], 6, 9)
    assert (rs, du, t_cov) == ([0, 2, 2, 2, 3, 9], [2, 0, 0, 1, 6, 0], 9)
    assert cr == [0, 0, 3, 4, 4, 4, 4, 4, 4]
    assert duration_runs_host([3.0, 3.0], 0, 5) == ([-1, -1], [0, 0], [-1] * 5, 0)
    assert duration_runs_host([3.0, 3.0], 2, 0) == ([0, 0], [0, 0], [], 0)
