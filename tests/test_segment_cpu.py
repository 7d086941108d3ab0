"""The segment crop's integer window rule (monotonic_align.segment_offset_host, the host restatement of
mtts_segment_crop_fwd's offset arithmetic) and the Trainer's out_size default.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

S = 16
WORDS = (0, 1, 2 ** 30, 2 ** 31 - 2)
HIST_N, HIST_MAX_OFF, HIST_SEED = 2048, 8, 20
# Binomial(2048, 1/8): mean 256, sigma = sqrt(2048 * 1/8 * 7/8) ~ 15 -> 5 sigma = 75
HIST_LO, HIST_HI = 256 - 75, 256 + 75


def hist_words() -> np.ndarray:
    """The seeded 31-bit words of the histogram checks (shared with tests/test_segment_gpu.py)."""
    return np.random.default_rng(HIST_SEED).integers(0, 2 ** 31 - 1, HIST_N, dtype=np.int64)


@pytest.mark.parametrize("t_y", [S - 3, S, S + 1, S + 2, S + 9])
@pytest.mark.parametrize("word", WORDS)
def test_segment_offset_host_corner_words(word, t_y):
    from matcha.utils.monotonic_align import segment_offset_host

    off, cut = segment_offset_host(word, t_y, S)
    max_off = max(t_y - S, 0)
    assert cut == min(t_y, S)
    assert 0 <= off <= max(max_off - 1, 0)  # max_off itself is never drawn (random.choice(range(0, max_off)))
    if max_off <= 1:
        assert off == 0
    assert off == (word * max_off) >> 31  # the rule itself, in plain integers
    assert off + cut <= t_y or t_y <= 0


def test_segment_offset_host_extremes_of_the_range():
    from matcha.utils.monotonic_align import segment_offset_host

    assert segment_offset_host(0, S + 9, S) == (0, S)
    assert segment_offset_host(2 ** 31 - 2, S + 9, S) == (8, S)  # the largest word reaches max_off - 1
    assert segment_offset_host(2 ** 31 - 2, S + 2, S) == (1, S)
    assert segment_offset_host(2 ** 30, S + 9, S) == (4, S)
    assert segment_offset_host(123456789, 0, S) == (0, 0)


def test_segment_offset_histogram_is_uniform():
    from matcha.utils.monotonic_align import segment_offset_host

    offs = np.array([segment_offset_host(int(w), S + HIST_MAX_OFF, S)[0] for w in hist_words()])
    assert offs.min() >= 0 and offs.max() <= HIST_MAX_OFF - 1  # offset 8 never appears
    bins = np.bincount(offs, minlength=HIST_MAX_OFF)
    assert len(bins) == HIST_MAX_OFF
    assert ((bins >= HIST_LO) & (bins <= HIST_HI)).all(), bins


def test_train_config_out_size_default():
    from matcha.training import TrainConfig

    assert TrainConfig().out_size is None
    assert TrainConfig(out_size=64).out_size == 64
