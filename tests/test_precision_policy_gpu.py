"""What the forward-precision policy launches: the precision and the split flags of every logged GEMM of linear_tm
and preln_ff_tm, forward and backward, in every mode (tests/test_precision_policy_cpu.py pins the decisions on the
host; this file pins that the launches follow them).  The backward is never the policy's: bf16 one plane in every
bf16 mode, wherever backward() is called."""
from __future__ import annotations

import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, T, C, HID = 2, 16, 64, 256  # M = 2 * 16 rows, K = N = 64, FF hidden 256


def _ops():
    from matcha.models.components import _ops as O

    return O


def _rand(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


@contextlib.contextmanager
def _split_on():
    O = _ops()
    old = O.set_weight_split(True)
    try:
        yield
    finally:
        O.set_weight_split(old)


def _mode(name):
    O = _ops()
    return {"plain": contextlib.nullcontext, "split": _split_on, "bf16x3": O.precise_forward,
            "bf16x6": lambda: O.precise_forward("bf16x6"), "fp32": lambda: O.precise_forward("fp32"),
            "parity": O.parity_policy}[name]()


@contextlib.contextmanager
def _logged():
    O = _ops()
    old, O.LAUNCH_LOG = O.LAUNCH_LOG, []
    try:
        yield O.LAUNCH_LOG
    finally:
        O.LAUNCH_LOG = old


def _launches(log):
    O = _ops()
    mask = O.GEMM_F_W_SPLIT | O.GEMM_F_A_SPLIT | O.GEMM_F_SPLIT3
    return [(e[3], e[5]["flags"] & mask) for e in log]


# mode -> (precision, split flags) of linear_tm's forward GEMM inside a bf16 autocast region
LINEAR_BF16 = {"plain": ("bf16", ()), "split": ("bf16", ("W",)), "bf16x3": ("bf16", ("W", "A")),
               "bf16x6": ("bf16", ("S3",)), "fp32": ("fp32", ()), "parity": ("bf16", ("W",))}


def _want(prec, flags):
    O = _ops()
    bits = {"W": O.GEMM_F_W_SPLIT, "A": O.GEMM_F_A_SPLIT, "S3": O.GEMM_F_SPLIT3}
    return ({"bf16": O.PREC_BF16, "fp32": O.PREC_FP32}[prec], sum(bits[f] for f in flags))


@pytest.mark.parametrize("amp", [True, False], ids=["autocast", "no_autocast"])
@pytest.mark.parametrize("mode", list(LINEAR_BF16))
def test_linear_tm_launches(mode, amp):
    O = _ops()
    x = _rand(B, T, C, seed=1).requires_grad_()
    w = _rand(C, C, seed=2, scale=C ** -0.5).requires_grad_()
    b = _rand(C, seed=3).requires_grad_()
    with _logged() as log:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp), _mode(mode):
            y = O.linear_tm(x, w, b)
        fwd = _launches(log)
        del log[:]
        y.square().sum().backward()  # after leaving the contexts, as the model does
        torch.cuda.synchronize()
        bwd = _launches(log)
    assert fwd == [_want(*LINEAR_BF16[mode]) if amp else (O.PREC_FP32, 0)], (mode, amp, fwd)
    assert bwd and all(e == (O.PREC_BF16 if amp else O.PREC_FP32, 0) for e in bwd), (mode, amp, bwd)
    assert all(torch.isfinite(t.grad).all() for t in (x, w, b))


def _ff_inputs():
    h = _rand(B, T, C, seed=11).requires_grad_()
    ps = [_rand(C, seed=12).add_(1.0), _rand(C, seed=13), _rand(HID, C, seed=14, scale=C ** -0.5), _rand(HID, seed=15),
          _rand(C, HID, seed=16, scale=HID ** -0.5), _rand(C, seed=17)]
    return h, [p.requires_grad_() for p in ps]


@pytest.mark.parametrize("mode,up_down", [("parity", ((), ("W",))), ("split", (("W",), ("W",)))])
def test_preln_ff_tm_launches(mode, up_down):
    """The FeedForward's GELU up-projection keeps one plane under the parity policy, not under the process-wide
    split alone; the down-projection is split in both."""
    O = _ops()
    if O._FF1_SPLIT:
        up_down = (("W",), ("W",))  # MTTS_PARITY_FF1_SPLIT=1: the policy splits the up-projection too
    h, (lnw, lnb, w1, b1, w2, b2) = _ff_inputs()
    with _logged() as log:
        with torch.autocast("cuda", dtype=torch.bfloat16), _mode(mode):
            y = O.preln_ff_tm(h, lnw, lnb, 1e-5, w1, b1, w2, b2)
        fwd = [(e[5]["act"],) + l for e, l in zip(log, _launches(log))]
        del log[:]
        y.square().sum().backward()
        torch.cuda.synchronize()
        bwd = _launches(log)
    assert fwd == [(O.ACT_GELU,) + _want("bf16", up_down[0]), (O.ACT_NONE,) + _want("bf16", up_down[1])], fwd
    assert bwd and all(e == (O.PREC_BF16, 0) for e in bwd), bwd


def test_backward_inside_precise_forward_is_the_same_backward():
    """The policy is read in the forward only: backward() called inside a precise_forward() block gives bitwise
    the gradients of backward() called after leaving it."""
    O = _ops()
    grads, launches = [], []
    for inside in (False, True):
        x = _rand(B, T, C, seed=1).requires_grad_()
        w = _rand(C, C, seed=2, scale=C ** -0.5).requires_grad_()
        b = _rand(C, seed=3).requires_grad_()
        h, ff = _ff_inputs()
        with _logged() as log:
            with torch.autocast("cuda", dtype=torch.bfloat16), O.precise_forward():
                y = O.preln_ff_tm(O.linear_tm(x, w, b) + h, *ff[:2], 1e-5, *ff[2:])
                del log[:]
                if inside:
                    y.square().sum().backward()
            if not inside:
                y.square().sum().backward()
            torch.cuda.synchronize()
            launches.append(_launches(log))
        grads.append([t.grad.clone() for t in (x, w, b, h, *ff)])
    assert launches[0] == launches[1] and launches[0] and all(e == (O.PREC_BF16, 0) for e in launches[0])
    for g0, g1 in zip(*grads):
        assert torch.isfinite(g0).all() and torch.equal(g0, g1)
