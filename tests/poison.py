"""Poisoned `torch.empty`: run code on buffers whose bytes are chosen by the test, not by the allocator.

The operator layer gets its outputs, saved activations and workspaces from `torch.empty` / `torch.empty_like`.
In a fresh process the caching allocator hands back zeros or tame floats, so a kernel that leaves part of a
buffer unwritten, reads a workspace slot before writing it, or masks stale data with `0 * x` passes every
arithmetic test and fails in a long run. `poisoned(byte)` makes the content of every such buffer explicit;
`run_under_fills` runs a function under several fills and demands bitwise identical, finite results.

    0x00 -> 0.0 / int 0                         (what a fresh process usually sees)
    0x7F -> 3.39e38 in fp32 and bf16 (finite), int32 2139062143, uint8 127
    0xFF -> NaN in fp32 and bf16, int32 -1, uint8 255

Imported like dropout_ref / norm_ref (tests/ is on sys.path); it needs nothing from conftest.
"""
from __future__ import annotations

import os

import torch

FILLS = (0x00, 0x7F, 0xFF)

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class poisoned:
    """Context manager: every tensor that `torch.empty` / `torch.empty_like` returns holds `byte` in every byte.

    Patches the two attributes of the `torch` module, which is how every call site in the project spells them
    (a `functools.partial(torch.empty, ...)` made inside the context included), and restores them on exit, also
    on error. The fill is an ordinary `fill_` kernel on the current stream through a uint8 view of the new
    tensor's storage, so it works for every dtype, for 0-dim tensors, and inside graph capture (where it becomes
    a node and is replayed). `count` is the number of allocations poisoned so far.
    """

    def __init__(self, byte: int):
        if not 0 <= int(byte) <= 0xFF:
            raise ValueError(f"fill byte out of range: {byte!r}")
        self.byte = int(byte)
        self.count = 0
        self._saved = None

    def _fill(self, t):
        if not isinstance(t, torch.Tensor) or t.layout != torch.strided:
            return t
        st = t.untyped_storage()
        n = st.nbytes()
        if n:
            self._saved[0](0, dtype=torch.uint8, device=t.device).set_(st, 0, (n,), (1,)).fill_(self.byte)
            self.count += 1
        return t

    def __enter__(self):
        real_empty, real_empty_like = torch.empty, torch.empty_like
        self._saved = (real_empty, real_empty_like)

        def empty(*args, **kwargs):
            return self._fill(real_empty(*args, **kwargs))

        def empty_like(*args, **kwargs):
            return self._fill(real_empty_like(*args, **kwargs))

        torch.empty, torch.empty_like = empty, empty_like
        _ACTIVE.append(self)
        return self

    def __exit__(self, *exc):
        _ACTIVE.remove(self)
        torch.empty, torch.empty_like = self._saved
        return False


def _as_int(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    if t.dim() == 0:
        t = t.reshape(1)
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    return t.view(_INT_VIEW[t.element_size()])


def difference(a: torch.Tensor, b: torch.Tensor) -> str | None:
    """None where `a` and `b` agree bit for bit (same shape and dtype too), else a sentence saying where not."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape/dtype {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    ne = _as_int(a) != _as_int(b)
    n = int(ne.sum())
    if n == 0:
        return None
    a1, b1 = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    flat = ne.reshape(-1).nonzero().reshape(-1)
    per = max(ne.numel() // max(a1.numel(), 1), 1)  # complex dtypes view as two ints per element
    first = int(flat[0]) // per
    idx = []
    rem = first
    for s in reversed(a.shape):
        idx.append(rem % s)
        rem //= s
    return (f"{n} of {ne.numel()} words differ in {tuple(a.shape)} {a.dtype}; first at {tuple(reversed(idx))}: "
            f"{a1[first].item()!r} vs {b1[first].item()!r}; last at flat {int(flat[-1]) // per}")


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape, same dtype and the same bits: compared through an integer view, so NaN equals the same NaN."""
    return difference(a, b) is None


def _selected_fills():
    # MTTS_POISON_FILLS=7f (or "7f,ff") restricts the non-zero fills, so a first run on a shared machine can
    # take them one at a time; the two 0x00 runs always happen. Unset: all of FILLS. A value that selects no
    # non-zero fill, or names a byte that is not one of FILLS, is an error: such a run must not report green.
    env = os.environ.get("MTTS_POISON_FILLS")
    if env is None:
        return FILLS[1:]
    try:
        want = {int(s, 16) for s in env.replace(",", " ").split()}
    except ValueError:
        want = None
    if not want or not want <= set(FILLS[1:]):
        raise ValueError(f"MTTS_POISON_FILLS={env!r}: expected one or more of "
                         + ", ".join(f"{f:02x}" for f in FILLS[1:]))
    return tuple(f for f in FILLS[1:] if f in want)


_ACTIVE = []


def current():
    """The innermost active poisoned() context (a case reads `.count` around a call to see what the call itself
    allocated, and `.byte` to check a region it documents as untouched)."""
    if not _ACTIVE:
        raise RuntimeError("no poisoned() context is active")
    return _ACTIVE[-1]


def run_under_fills(fn, seed: int = 1234):
    """Call `fn()` under 0x00, 0x00 again, 0x7F and 0xFF; it returns a flat list of tensors (None is skipped).

    Each call is preceded by torch.cuda.manual_seed(seed), which replays the ops' dropout seeds. Asserts that
    every run poisoned at least one allocation, that the two 0x00 runs agree bit for bit (determinism: the
    precondition for what follows, asserted, not skipped), and that the 0x7F and 0xFF runs are finite and agree
    bit for bit with the 0x00 run. Returns the outputs of the first run.
    """
    fills = _selected_fills()

    def once(byte):
        torch.cuda.manual_seed(seed)
        with poisoned(byte) as p:
            outs = fn()
            outs = [o for o in outs if o is not None]
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            outs = [o.detach().clone() for o in outs]
        assert p.count >= 1, "the case allocated nothing through torch.empty / torch.empty_like: it proves nothing"
        assert outs, "the case returned no tensor"
        return outs

    base = once(0x00)
    again = once(0x00)
    assert len(base) == len(again)
    for i, (a, b) in enumerate(zip(base, again)):
        d = difference(a, b)
        assert d is None, f"output {i} is not deterministic under fill 0x00: {d}"
    for byte in fills:
        got = once(byte)
        assert len(got) == len(base)
        for i, (a, b) in enumerate(zip(got, base)):
            if a.is_floating_point() or a.is_complex():
                where = (~torch.isfinite(a)).reshape(-1).nonzero().reshape(-1)
                assert where.numel() == 0, (f"output {i} has {where.numel()} non-finite of {a.numel()} elements under "
                                            f"fill {byte:#04x}, first at flat index {int(where[0])}")
            d = difference(a, b)
            assert d is None, f"output {i} depends on uninitialised memory (fill {byte:#04x} vs 0x00): {d}"
    return base
