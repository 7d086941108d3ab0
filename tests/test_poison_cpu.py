"""The poisoned-allocation harness itself (tests/poison.py), on CPU tensors: no GPU needed."""
import functools
import math

import pytest
import torch

import poison as P

REAL_EMPTY, REAL_EMPTY_LIKE = torch.empty, torch.empty_like


@pytest.fixture(autouse=True)
def _all_fills(monkeypatch):
    monkeypatch.delenv("MTTS_POISON_FILLS", raising=False)


def test_fills_are_the_three_documented_bytes():
    assert P.FILLS == (0x00, 0x7F, 0xFF)


def test_byte_patterns_per_dtype():
    with P.poisoned(0xFF):
        f, h, i, u = (torch.empty(5, dtype=d) for d in (torch.float32, torch.bfloat16, torch.int32, torch.uint8))
    assert torch.isnan(f).all() and torch.isnan(h).all()
    assert (i == -1).all() and (u == 255).all()
    with P.poisoned(0x7F):
        f, h, i, u = (torch.empty(5, dtype=d) for d in (torch.float32, torch.bfloat16, torch.int32, torch.uint8))
    assert torch.isfinite(f).all() and torch.isfinite(h).all()
    assert math.isclose(float(f[0]), 3.39e38, rel_tol=2e-3) and math.isclose(float(h[0]), 3.39e38, rel_tol=2e-3)
    assert (i == 2139062143).all() and (u == 127).all()
    with P.poisoned(0x00):
        f, i = torch.empty(3, 4), torch.empty((2, 2), dtype=torch.int32)
    assert (f == 0).all() and (i == 0).all()


def test_zero_dim_noncontiguous_like_and_partial():
    src = torch.arange(24.0).reshape(4, 6)[:, ::2]  # not contiguous, not dense
    assert not src.is_contiguous()
    with P.poisoned(0xFF) as p:
        s = torch.empty((), dtype=torch.float32)
        like = torch.empty_like(src)
        like16 = torch.empty_like(src, dtype=torch.bfloat16)
        perm = torch.empty_like(torch.zeros(2, 3, 4).permute(2, 0, 1))  # dense, keeps the permuted strides
        new = functools.partial(torch.empty, dtype=torch.float32)  # made at call time, as in _TimeMLP
        part = new(3, 2)
        nothing = torch.empty(0)
    assert s.dim() == 0 and math.isnan(float(s))
    assert like.shape == src.shape and like.is_contiguous() and torch.isnan(like).all()
    assert like16.dtype == torch.bfloat16 and torch.isnan(like16).all()
    assert perm.shape == (4, 2, 3) and torch.isnan(perm).all()
    assert part.shape == (3, 2) and torch.isnan(part).all()
    assert nothing.numel() == 0
    assert p.count == 5  # the zero-byte tensor has nothing to poison and is not counted
    assert torch.equal(src, torch.arange(24.0).reshape(4, 6)[:, ::2])  # the source is untouched


def test_restores_on_exit_and_after_an_exception():
    with P.poisoned(0x7F):
        assert torch.empty is not REAL_EMPTY and torch.empty_like is not REAL_EMPTY_LIKE
    assert torch.empty is REAL_EMPTY and torch.empty_like is REAL_EMPTY_LIKE
    with pytest.raises(RuntimeError, match="boom"):
        with P.poisoned(0xFF):
            torch.empty(2)
            raise RuntimeError("boom")
    assert torch.empty is REAL_EMPTY and torch.empty_like is REAL_EMPTY_LIKE
    with pytest.raises(ValueError):
        P.poisoned(256)


def test_nested_contexts_unwind_in_order():
    with P.poisoned(0x00) as outer:
        with P.poisoned(0xFF) as inner:
            assert torch.isnan(torch.empty(2)).all()
        assert (torch.empty(2) == 0).all()
    assert inner.count == 1 and outer.count == 2  # the inner wrapper calls the outer one, which fills first
    assert torch.empty is REAL_EMPTY


def test_allocation_count():
    with P.poisoned(0x00) as p:
        assert p.count == 0
        a = torch.empty(4)
        torch.empty_like(a)
        torch.zeros(4)  # not patched, not counted
        assert p.count == 2
    torch.empty(4)
    assert p.count == 2


def test_bits_equal_compares_nans_by_pattern_and_says_where():
    nan = torch.tensor([1.0, float("nan"), 3.0])
    assert P.bits_equal(nan, nan.clone())
    assert not torch.equal(nan, nan.clone())  # what a value comparison would have said
    other = nan.clone()
    other[2] = 4.0
    assert not P.bits_equal(nan, other)
    assert "first at (2,)" in P.difference(nan, other)
    assert not P.bits_equal(torch.zeros(3), torch.zeros(3, dtype=torch.bfloat16))
    assert not P.bits_equal(torch.zeros(3), torch.zeros(1, 3))
    assert not P.bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))  # bits, not values
    assert P.bits_equal(torch.tensor(2.0), torch.tensor(2.0))  # 0-dim
    m = torch.zeros(2, 3, dtype=torch.bfloat16)
    m2 = m.clone()
    m2[1, 1] = 1
    assert "first at (1, 1)" in P.difference(m, m2)
    assert P.bits_equal(torch.tensor([True, False]), torch.tensor([True, False]))


def _toy(written):
    def fn():
        out = torch.empty(8)
        out[:written] = torch.arange(float(written))
        return [out]
    return fn


def test_teeth_half_written_buffer_fails():
    with pytest.raises(AssertionError, match="fill 0x7f"):
        P.run_under_fills(_toy(4))
    assert torch.empty is REAL_EMPTY


def test_fully_written_buffer_passes():
    (out,) = P.run_under_fills(_toy(8))
    assert torch.equal(out, torch.arange(8.0))


def test_teeth_zero_times_stale_fails_only_under_nan(monkeypatch):
    # 0 * x masks 3.39e38 but not NaN: the 0xFF fill is the one that catches it.
    def fn():
        ws = torch.empty(4)
        return [torch.ones(4) + 0.0 * ws]
    with pytest.raises(AssertionError, match="non-finite.*fill 0xff"):
        P.run_under_fills(fn)
    monkeypatch.setenv("MTTS_POISON_FILLS", "7f")
    P.run_under_fills(fn)  # restricted to 0x7F it passes, which is why the default runs every fill


@pytest.mark.parametrize("value", ["00", "", "7e", "7f,zz", "0x7f 00"])
def test_a_selection_that_runs_no_poison_or_an_unknown_byte_is_an_error(monkeypatch, value):
    monkeypatch.setenv("MTTS_POISON_FILLS", value)
    with pytest.raises(ValueError, match="MTTS_POISON_FILLS"):
        P.run_under_fills(_toy(8))
    assert torch.empty is REAL_EMPTY


def test_current_context_is_the_innermost_one():
    with pytest.raises(RuntimeError):
        P.current()
    with P.poisoned(0x7F) as outer:
        assert P.current() is outer and P.current().byte == 0x7F
        with P.poisoned(0xFF) as inner:
            assert P.current() is inner
        assert P.current() is outer
        before = P.current().count
        torch.empty(3)
        assert P.current().count - before == 1
    with pytest.raises(RuntimeError):
        P.current()


def test_a_case_that_allocates_nothing_fails():
    with pytest.raises(AssertionError, match="proves nothing"):
        P.run_under_fills(lambda: [torch.zeros(3)])


def test_nondeterministic_case_fails_the_precondition():
    calls = []

    def fn():
        calls.append(1)
        out = torch.empty(2)
        out[:] = float(len(calls))
        return [out]
    with pytest.raises(AssertionError, match="not deterministic"):
        P.run_under_fills(fn)


def test_run_order_is_zero_zero_7f_ff():
    seen = []

    def fn():
        t = torch.empty(1, dtype=torch.uint8)
        seen.append(int(t))
        t.zero_()
        return [t]
    P.run_under_fills(fn)
    assert seen == [0x00, 0x00, 0x7F, 0xFF]
